"""Restatements of the attention rollout for the tests (numpy / torch on the host; nothing here imports clibd_amd):

  * fp64 from bf16 qkv: P -> head fusion -> discard with the stated tie rule -> the column-broadcast normalisation -> the chain, as the
    reference's full matrix product (scripts/result/representation_visualization/*.py, `rollout`);
  * an fp32 emulation of the same formulas, the yardstick of the device's gates: the device may be off from fp64 by at most GATE x the
    emulation's error on the same inputs (the margin covers another summation order and the exp2 form of the exponential).

Inputs are regenerated from seeds (`synth_qkv`, `synth_maps`) by the fixture's maker and by the tests alike.
"""
import numpy as np
import torch

GATE = 4.0
VIT_WINDOW = slice(1, -6)
DNA_WINDOW = slice(1, None)


# ---- inputs from seeds --------------------------------------------------------------------------------------------------------------------
def synth_qkv(seed, B: int, S: int, heads: int, sigma: float = 1.0) -> torch.Tensor:
    """bf16 [B * S, 3 * 64 * heads]: N(0, sigma^2) entries from numpy's legacy RandomState (seed: an int or a list of ints)"""
    rs = np.random.RandomState(seed)
    x = (rs.randn(B * S, 3 * 64 * heads) * sigma).astype(np.float32)
    return torch.from_numpy(x).to(torch.bfloat16)


def synth_maps(seed, L: int, S: int) -> np.ndarray:
    """fp32 [L, S, S] single-head "attentions": a row-wise softmax of N(0, 1.5^2) logits computed in fp64, rounded once to fp32"""
    rs = np.random.RandomState(seed)
    z = rs.randn(L, S, S) * 1.5
    e = np.exp(z - z.max(axis=-1, keepdims=True))
    return (e / e.sum(axis=-1, keepdims=True)).astype(np.float32)


# ---- P and the fusion -----------------------------------------------------------------------------------------------------------------------
def split_qk(qkv: torch.Tensor, B: int, S: int, heads: int, dtype):
    """(q, k) [B, heads, S, 64] of a packed [B * S, 3 H] operand, exactly widened from bf16"""
    H = 64 * heads
    x = qkv.detach().cpu().to(torch.float32).to(dtype).view(B, S, 3, heads, 64)
    return x[:, :, 0].permute(0, 2, 1, 3), x[:, :, 1].permute(0, 2, 1, 3)


def probs(qkv: torch.Tensor, B: int, S: int, heads: int, dtype=torch.float64) -> torch.Tensor:
    """softmax(q k^T / sqrt(64)) [B, heads, S, S] in `dtype` (fp64: the reference; fp32: the emulation)"""
    q, k = split_qk(qkv, B, S, heads, dtype)
    s = (q @ k.transpose(-1, -2)) * 0.125
    s = s - s.max(dim=-1, keepdim=True)[0]
    e = torch.exp(s)
    return e / e.sum(dim=-1, keepdim=True)


def fuse(P: torch.Tensor, fusion: str) -> torch.Tensor:
    if fusion == "mean":
        return P.mean(dim=1)
    if fusion == "max":
        return P.max(dim=1)[0]
    if fusion == "min":
        return P.min(dim=1)[0]
    raise ValueError(fusion)


def fused_maps(qkv, B, S, heads, fusion, dtype=torch.float64) -> np.ndarray:
    """[B, S, S] numpy in `dtype`"""
    return fuse(probs(qkv, B, S, heads, dtype), fusion).numpy()


# ---- discard --------------------------------------------------------------------------------------------------------------------------------
def discard_count(S: int, ratio: float) -> int:
    return int(S * S * ratio)


def discard_pattern(F: np.ndarray, k: int) -> np.ndarray:
    """bool [S, S]: the entries the discard zeroes.  The k smallest by (value, flat index) — every entry below the k-th smallest value, the
    entries equal to it in ascending flat index until k are taken — without flat index 0, which still counts among the k."""
    flat = F.reshape(-1)
    order = np.argsort(flat, kind="stable")[:k]
    z = np.zeros(flat.shape, dtype=bool)
    z[order] = True
    z[0] = False
    return z.reshape(F.shape)


def discard(F: np.ndarray, k: int) -> np.ndarray:
    out = F.copy()
    out[discard_pattern(F, k)] = 0
    return out


def boundary(F: np.ndarray, k: int):
    """(t, gap): the k-th smallest value and the relative distance to the (k + 1)-th ((inf) when k is 0 or S * S)"""
    flat = np.sort(F.reshape(-1).astype(np.float64))
    if k <= 0 or k >= flat.size:
        return (flat[k - 1] if k > 0 else 0.0), np.inf
    return flat[k - 1], (flat[k] - flat[k - 1]) / flat[k - 1]


# ---- the chain ------------------------------------------------------------------------------------------------------------------------------
def chain_matrix(maps, dtype=np.float64) -> np.ndarray:
    """the reference's loop on discarded maps [L][S, S] in its order of application: a = (F + I) / 2; a = a / a.sum(-1) with the divisor
    broadcast over the LAST axis (column j over the sum of row j); result = a @ result.  Returns mask = result[0, 1:] / max."""
    S = maps[0].shape[-1]
    result = np.eye(S, dtype=dtype)
    I = np.eye(S, dtype=dtype)
    for F in maps:
        a = (F.astype(dtype) + I) / 2
        a = a / a.sum(axis=-1)[None, :]
        result = a @ result
    mask = result[0, 1:]
    return mask / mask.max()


def chain_vector32(maps) -> np.ndarray:
    """the device's formula in fp32: r[j] = (sum_k F[j, k] + 1) / 2, v <- e0, for l = L - 1 .. 0: v[j] <- (sum_i v[i] a_l[i, j]) / r_l[j]"""
    f = np.float32
    S = maps[0].shape[-1]
    v = np.zeros(S, dtype=f)
    v[0] = 1
    I = np.eye(S, dtype=f)
    for F in reversed(list(maps)):
        F = F.astype(f)
        r = (F.sum(axis=-1, dtype=f) + f(1)) * f(0.5)
        a = (F + I) * f(0.5)
        v = ((v[None, :] @ a)[0] / r).astype(f)
    mask = v[1:]
    return mask / mask.max()


def select_layers(n_layers: int, layer_idx=None, window: slice = VIT_WINDOW):
    layers = list(range(n_layers))
    return layers[window] if layer_idx is None else layers[layer_idx:layer_idx + 1]


# ---- composed -------------------------------------------------------------------------------------------------------------------------------
def rollout64(fused, ratio: float, patterns=None) -> np.ndarray:
    """fp64 mask [S - 1] of one image from its fp64 fused maps [L][S, S]; `patterns` (bool [L][S, S]) replaces the discard's own selection
    (the composed test evaluates the fp64 chain on the device's zero pattern)"""
    S = fused[0].shape[-1]
    k = discard_count(S, ratio)
    out = []
    for l, F in enumerate(fused):
        if patterns is None:
            out.append(discard(np.asarray(F, dtype=np.float64), k))
        else:
            G = np.asarray(F, dtype=np.float64).copy()
            G[patterns[l]] = 0
            out.append(G)
    return chain_matrix(out)


def rollout32(fused32, ratio: float, patterns=None) -> np.ndarray:
    """the fp32 emulation of the same: fp32 fused maps, the same discard rule (or the given patterns), the fp32 vector chain"""
    S = fused32[0].shape[-1]
    k = discard_count(S, ratio)
    out = []
    for l, F in enumerate(fused32):
        F = np.asarray(F, dtype=np.float32)
        if patterns is None:
            out.append(discard(F, k))
        else:
            G = F.copy()
            G[patterns[l]] = 0
            out.append(G)
    return chain_vector32(out)


def rel_err(x, ref64) -> float:
    """max over the entries of |x - ref| / ref (ref > 0 asserted)"""
    ref64 = np.asarray(ref64, dtype=np.float64)
    assert (ref64 > 0).all()
    return float((np.abs(np.asarray(x, dtype=np.float64) - ref64) / ref64).max())


def abs_err(x, ref64) -> float:
    return float(np.abs(np.asarray(x, dtype=np.float64) - np.asarray(ref64, dtype=np.float64)).max())
