"""GPU checks of the attention rollout (clibd_amd.rollout, include/clibd_hip_rollout.h) against the restatements of tests/rollout_reference.py.

Gates: the device may be off from the fp64 restatement by at most GATE = 4 x the error of the fp32 same-formula emulation on the same inputs
(relative per entry for the fused maps, absolute for the normalised mask); the discard compares under torch.equal with the host's result
on the same fp32 bits; batches and repeated runs compare bit for bit.

Measured on an MI355X (device error / emulation error): see DESIGN §3.10."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import rollout_reference as RR  # noqa: E402

pytestmark = pytest.mark.gpu
FUSIONS = ("mean", "max", "min")


@pytest.fixture(scope="module")
def golden():
    return torch.load(ROOT / "tests" / "golden" / "rollout_golden.pt", weights_only=False)


_maps_ref = {}


def maps_ref(seed, B, S, heads, fusion):
    """(qkv, F fp64, F fp32 emulation) of one seeded case, computed once"""
    key = (seed if isinstance(seed, int) else tuple(seed), B, S, heads, fusion)
    if key not in _maps_ref:
        qkv = RR.synth_qkv(seed, B, S, heads)
        _maps_ref[key] = (qkv, RR.fused_maps(qkv, B, S, heads, fusion), RR.fused_maps(qkv, B, S, heads, fusion, torch.float32))
    return _maps_ref[key]


def padded(maps: np.ndarray, dev, fill=7.0):
    """device fp32 [..., S, ld] buffer of host maps [..., S, S]; the padding columns hold `fill`, which no entry may read"""
    from clibd_amd import ops

    S = maps.shape[-1]
    buf = torch.full(maps.shape[:-1] + (ops.rollout_ld(S),), fill, dtype=torch.float32)
    buf[..., :S] = torch.from_numpy(np.ascontiguousarray(maps, dtype=np.float32))
    return buf.to(dev)


# ---- 1. fused maps ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fusion", FUSIONS)
@pytest.mark.parametrize("B,S,heads", [(1, 197, 12), (3, 133, 12), (2, 20, 8), (2, 17, 3), (1, 256, 2), (1, 33, 2), (2, 32, 1), (1, 2, 1)])
def test_fused_maps_against_fp64(dev, B, S, heads, fusion):
    from clibd_amd import rollout as R

    qkv, F64, F32 = maps_ref([11, S], B, S, heads, fusion)
    F = R.fused_attention_maps(qkv.to(dev), B, S, heads, fusion)
    assert F.shape == (B, S, S) and F.dtype == torch.float32
    got = F.cpu().numpy()
    assert (F64 > 0).all()
    emu, err = RR.rel_err(F32, F64), RR.rel_err(got, F64)
    print(f"fused {fusion} B={B} S={S} heads={heads}: device {err:.3e}, emulation {emu:.3e}, ratio {err / emu:.2f}")
    assert err <= RR.GATE * emu
    if heads == 1:      # the mean over one head is that head: all three fusions give the same bits
        other = R.fused_attention_maps(qkv.to(dev), B, S, heads, "max")
        assert torch.equal(F, other)


# ---- 2. discard ---------------------------------------------------------------------------------------------------------------------------
def distinct_maps(seed, B, S):
    """fp32 [B, S, S], every entry of a map distinct and positive"""
    rs = np.random.RandomState(seed)
    out = np.empty((B, S * S), dtype=np.float32)
    for b in range(B):
        out[b] = (rs.permutation(S * S).astype(np.float64) + 1 + 0.5 * rs.rand(S * S)).astype(np.float32) / np.float32(S * S)
        assert len(np.unique(out[b])) == S * S
    return out.reshape(B, S, S)


def run_discard(maps: np.ndarray, k: int, dev):
    """(device result [B, S, S], untouched padding?, selection record) of the in-place discard on padded copies"""
    from clibd_amd import ops

    S = maps.shape[-1]
    buf = padded(maps, dev)
    rec = ops.rollout_discard_(buf, S, k)
    out = buf.cpu()
    return out[..., :S], bool((out[..., S:] == 7.0).all()), rec.cpu().numpy()


@pytest.mark.parametrize("ratio", [0.0, 0.5, 0.9, 1.0])
@pytest.mark.parametrize("B,S", [(1, 197), (3, 133), (3, 17), (1, 256), (3, 2)])
def test_discard_is_exact(dev, B, S, ratio):
    maps = distinct_maps([2, S], B, S)
    k = RR.discard_count(S, ratio)
    got, pad_ok, rec = run_discard(maps, k, dev)
    want = np.stack([RR.discard(maps[b], k) for b in range(B)])
    assert torch.equal(got, torch.from_numpy(want)) and pad_ok
    zeroed = (got == 0).reshape(B, -1).sum(dim=1).tolist()
    assert all(z in (k, k - 1) for z in zeroed) if k else zeroed == [0] * B
    if k:
        for b in range(B):
            t = np.sort(maps[b].reshape(-1))[k - 1]
            assert rec[b].tolist() == [int(t.view(np.uint32)), k - 1, 1, k]


def test_discard_index_zero_and_ties(dev):
    S = 33
    k = RR.discard_count(S, 0.9)
    base = distinct_maps(3, 1, S)[0]
    lo, hi = base.copy(), base.copy()
    lo[0, 0] = base.min() / 2          # [0, 0] the smallest: it counts among the k, so k - 1 entries are zeroed
    hi[0, 0] = base.max() * 2          # [0, 0] the largest: k entries are zeroed
    zeros = base.copy()
    zeros.reshape(-1)[np.random.RandomState(4).permutation(S * S)[: k + 57]] = 0      # more than k exact zeros
    quant = np.ceil(distinct_maps(5, 1, S)[0] * 64).astype(np.float32) / 64           # 1/64 steps: ties straddle the boundary
    flat = np.sort(quant.reshape(-1))
    assert flat[k - 1] == flat[k] and (quant == flat[k - 1]).sum() > 1 and flat[k - 1] > flat[0]
    stack = np.stack([lo, hi, zeros, quant])
    got, pad_ok, rec = run_discard(stack, k, dev)
    want = np.stack([RR.discard(m, k) for m in stack])
    assert torch.equal(got, torch.from_numpy(want)) and pad_ok
    nz = (torch.from_numpy(stack) != 0).reshape(4, -1).sum(dim=1) - (got != 0).reshape(4, -1).sum(dim=1)      # newly zeroed
    assert nz[0] == k - 1 and got[0, 0, 0] == lo[0, 0] and nz[1] == k and got[1, 0, 0] == hi[0, 0]
    assert nz[2] == 0 and rec[2, 0] == 0                                      # the k smallest are zeros already: nothing changes
    t = flat[k - 1]
    below, equal = int((quant < t).sum()), int((quant == t).sum())
    assert rec[3].tolist() == [int(t.view(np.uint32)), below, k - below, k] and 0 < k - below < equal
    kept = np.nonzero((quant == t).reshape(-1) & (got[3].reshape(-1).numpy() != 0))[0]
    gone = np.nonzero((quant == t).reshape(-1) & (got[3].reshape(-1).numpy() == 0))[0]
    assert len(gone) == k - below and gone.max() < kept.min()                # ascending flat index until k are taken


# ---- 3. chain -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 5, 11])
@pytest.mark.parametrize("B,S", [(2, 197), (1, 133), (2, 17), (1, 2), (1, 256)])
def test_chain_against_fp64(dev, B, S, L):
    from clibd_amd import ops

    k = RR.discard_count(S, 0.5 if S > 2 else 0.0)
    maps = np.stack([[RR.discard(m, k) for m in RR.synth_maps([7, S, L, b], L, S)] for b in range(B)], axis=1)      # [L, B, S, S]
    got = ops.rollout_chain(padded(maps, dev), S).cpu().numpy()
    assert got.shape == (B, S - 1)
    for b in range(B):
        m64 = RR.chain_matrix([maps[l, b] for l in range(L)])
        emu, err = RR.abs_err(RR.chain_vector32([maps[l, b] for l in range(L)]), m64), RR.abs_err(got[b], m64)
        print(f"chain B={B} S={S} L={L} b={b}: device {err:.3e}, emulation {emu:.3e}, ratio {err / max(emu, 1e-30):.2f}")
        assert err <= RR.GATE * emu


# ---- 4. composed, from qkv ------------------------------------------------------------------------------------------------------------------
def device_pipeline(qkvs, B, S, heads, fusion, ratio, dev):
    """(mask [B, S - 1], zero patterns bool [L, B, S, S], fused maps [L, B, S, S]) of the device path on the layers' qkv"""
    from clibd_amd import ops
    from clibd_amd import rollout as R

    maps = torch.empty((len(qkvs), B, S, ops.rollout_ld(S)), dtype=torch.float32, device=dev)
    for l, q in enumerate(qkvs):
        ops.attn_fused_maps(q.to(dev), B, S, heads, R.FUSIONS[fusion], out=maps[l])
    fused = maps[..., :S].cpu().numpy().copy()
    ops.rollout_discard_(maps, S, RR.discard_count(S, ratio))
    zero = (maps[..., :S] == 0).cpu().numpy()
    return ops.rollout_chain(maps, S).cpu().numpy(), zero, fused


def check_band(F64, zero_dev, k, tau, limit):
    """the device's zero pattern may differ from the fp64 one only where |F64 - t| <= tau t; that band may hold at most `limit` entries"""
    t, _ = RR.boundary(F64, k)
    want = RR.discard_pattern(F64, k)
    band = np.abs(F64 - t) <= tau * t
    assert not ((want != zero_dev) & ~band).any()
    assert limit is None or band.sum() <= limit, band.sum()
    assert zero_dev.sum() in (k, k - 1)
    return int(band.sum()), int((want != zero_dev).sum())


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("S,fusion", [(197, "max"), (133, "min"), (197, "mean")])
def test_composed_from_qkv(dev, S, fusion, seed):
    heads, L, ratio = 12, 5, 0.9
    k = RR.discard_count(S, ratio)
    refs = [maps_ref([21, seed, S, l], 1, S, heads, fusion) for l in range(L)]
    mask, zero, fused = device_pipeline([r[0] for r in refs], 1, S, heads, fusion, ratio, dev)
    worst_band = flips = 0
    for l, (_, F64, F32) in enumerate(refs):
        tau = RR.GATE * RR.rel_err(F32, F64)
        assert RR.rel_err(fused[l, 0], F64) <= tau
        nb, nf = check_band(F64[0], zero[l, 0], k, tau, 8)
        worst_band, flips = max(worst_band, nb), flips + nf
    pats = [zero[l, 0] for l in range(L)]
    m64 = RR.rollout64([r[1][0] for r in refs], ratio, pats)
    emu, err = RR.abs_err(RR.rollout32([r[2][0] for r in refs], ratio, pats), m64), RR.abs_err(mask[0], m64)
    print(f"composed S={S} {fusion} seed={seed}: band <= {worst_band} entries, {flips} flips; mask device {err:.3e}, emulation {emu:.3e}, ratio {err / emu:.2f}")
    assert err <= RR.GATE * emu


# ---- 5. goldens -----------------------------------------------------------------------------------------------------------------------------
def test_golden_a_from_qkv(dev, golden):
    """the reference's own masks, from qkv through the whole device path: both windows and reshapes, three fusions, ratios 0.9 and 0,
    layer_idx None and 3.  The reference ran in fp32 on fp32 probabilities: its own distance to the fp64 restatement is added to the gate."""
    cfg, seed = golden["A"]["cfg"], golden["A"]["seed"]
    S, heads, NL = cfg["S"], cfg["heads"], cfg["layers"]
    qkvs = [RR.synth_qkv([seed, l], 1, S, heads) for l in range(NL)]
    f64 = {f: [RR.fused_maps(q, 1, S, heads, f)[0] for q in qkvs] for f in cfg["fusions"]}
    f32 = {f: [RR.fused_maps(q, 1, S, heads, f, torch.float32)[0] for q in qkvs] for f in cfg["fusions"]}
    for (kind, fusion, ratio, li), ref in golden["A"]["masks"].items():
        layers = RR.select_layers(NL, li, RR.VIT_WINDOW if kind == "vit" else RR.DNA_WINDOW)
        mask, zero, _ = device_pipeline([qkvs[l] for l in layers], 1, S, heads, fusion, ratio, dev)
        k = RR.discard_count(S, ratio)
        for j, l in enumerate(layers):     # the maker asserted gaps of 64 x the emulation error: the patterns agree exactly
            assert np.array_equal(zero[j, 0], RR.discard_pattern(f64[fusion][l], k))
        m64 = RR.rollout64([f64[fusion][l] for l in layers], ratio)
        emu = RR.abs_err(RR.rollout32([f32[fusion][l] for l in layers], ratio), m64)
        own = RR.abs_err(ref.reshape(-1), m64)
        err64, err = RR.abs_err(mask[0], m64), RR.abs_err(mask[0], ref.reshape(-1))
        print(f"golden A {kind} {fusion} {ratio} {li}: device vs fp64 {err64:.3e} (emulation {emu:.3e}), vs the reference {err:.3e} (its own error {own:.3e})")
        assert err64 <= RR.GATE * emu and err <= RR.GATE * emu + own


def test_golden_b_maps_through_discard_and_chain(dev, golden):
    from clibd_amd import ops
    from clibd_amd import rollout as R

    for kind, window in (("vit", RR.VIT_WINDOW), ("dna", RR.DNA_WINDOW)):
        g = golden["B"][kind]
        S = g["S"]
        maps = RR.synth_maps(g["seed"], g["layers"], S)
        layers = RR.select_layers(g["layers"], None, window)
        k = RR.discard_count(S, g["ratio"])
        buf = padded(maps[layers][:, None], dev)
        ops.rollout_discard_(buf, S, k)
        for j, l in enumerate(layers):        # the same fp32 bits on both sides: torch.topk's own index set, exactly
            z = np.unpackbits(g["patterns"][l])[:S * S].astype(bool).reshape(S, S)
            want = maps[l].copy()
            want[z] = 0
            assert torch.equal(buf[j, 0, :, :S].cpu(), torch.from_numpy(want))
        mask = ops.rollout_chain(buf, S).cpu().numpy()[0]
        again = R.rollout_from_maps(torch.from_numpy(maps[layers][:, None]).to(dev), g["ratio"]).cpu().numpy()[0]
        assert np.array_equal(mask, again)
        m64 = RR.rollout64([maps[l].astype(np.float64) for l in layers], g["ratio"])
        emu = RR.abs_err(RR.rollout32([maps[l] for l in layers], g["ratio"]), m64)
        own = RR.abs_err(g["mask"].reshape(-1), m64)
        err64, err = RR.abs_err(mask, m64), RR.abs_err(mask, g["mask"].reshape(-1))
        print(f"golden B {kind}: device vs fp64 {err64:.3e} (emulation {emu:.3e}), vs the reference {err:.3e} (its own error {own:.3e})")
        assert err64 <= RR.GATE * emu and err <= RR.GATE * emu + own


# ---- 6. batches and repeats ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,heads,fusion", [(197, 12, "min"), (33, 2, "mean")])
def test_batch_independence_and_repeatability(dev, S, heads, fusion):
    from clibd_amd import rollout as R

    B, L, ratio = 3, 3, 0.9
    qkvs = [RR.synth_qkv([31, S, l], B, S, heads).to(dev) for l in range(L)]

    def run(rows):
        maps = torch.stack([R.fused_attention_maps(q.view(B, S, -1)[rows].reshape(len(rows) * S, -1).contiguous(), len(rows), S, heads, fusion)
                            for q in qkvs])
        return maps, R.rollout_from_maps(maps, ratio)

    maps3, mask3 = run([0, 1, 2])
    maps3b, mask3b = run([0, 1, 2])
    assert torch.equal(maps3, maps3b) and torch.equal(mask3, mask3b)          # two runs: the same bits
    for b in range(B):
        maps1, mask1 = run([b])
        assert torch.equal(maps1[:, 0], maps3[:, b]) and torch.equal(mask1[0], mask3[b])
    assert not torch.equal(mask3[0], mask3[1])


# ---- 7. towers, end to end ------------------------------------------------------------------------------------------------------------------
def _peaky(om):
    """query / key / qkv weights of N(0, 0.09^2): scores of order one (the default N(0, 0.02^2) gives nearly uniform attention), and
    adapters that do something"""
    with torch.no_grad():
        for n, p in om.named_parameters():
            if n.endswith(("qkv.weight", "query.weight", "key.weight", "query.w.weight")):
                p.normal_(0, 0.09)
            if "linear_b_" in n or ".w_b." in n:
                p.normal_(0, 0.02)


def _oracle_masks(O, om, x, layers, heads, fusion, monkeypatch):
    """the rollout (ratio 0) of the oracle's own q and k, captured by a test-side wrapper of its attention_core: (fp32 mode, bf16 mode)"""
    out = []
    for mode in ("fp32", "bf16"):
        seen = []
        inner = O.attention_core

        def spy(q, k, v, *a, **kw):
            seen.append((q.detach(), k.detach()))
            return inner(q, k, v, *a, **kw)

        monkeypatch.setattr(O, "attention_core", spy)
        with torch.no_grad(), O.precision(mode):
            om(x)
        monkeypatch.setattr(O, "attention_core", inner)
        fused = []
        for l in layers:
            q, k = seen[l]
            if mode == "bf16":
                q, k = q.to(torch.bfloat16), k.to(torch.bfloat16)
            q, k = q.to(torch.float32).to(torch.float64), k.to(torch.float32).to(torch.float64)
            s = (q @ k.transpose(-1, -2)) * 0.125
            fused.append(RR.fuse(torch.softmax(s, dim=-1), fusion).numpy())
        B = fused[0].shape[0]
        out.append(np.stack([RR.rollout64([f[b] for f in fused], 0.0) for b in range(B)]))
    return out


def _tower_case(dev, m, om, O, x, kind, heads, fusion, monkeypatch):
    from clibd_amd import rollout as R

    cls = R.VITAttentionRollout if kind == "vit" else R.BarcodeBERTAttentionRollout
    window = RR.VIT_WINDOW if kind == "vit" else RR.DNA_WINDOW
    B = x.shape[0]
    tower = m.tower()
    tower.training = False
    with torch.no_grad():
        _, state = tower._forward((x.to(dev),) if kind == "vit" else (x.to(dev), None, None), True)
    recorded = [r["qkv"].cpu() for r in state["saved"]]
    del state
    NL = len(recorded)
    S = recorded[0].shape[0] // B
    for li, ratio in ((None, 0.9), (None, 0.0), (NL - 1, 0.9)):
        layers = RR.select_layers(NL, li, window)
        ro = cls(m, head_fusion=fusion, discard_ratio=ratio)
        got = ro(x.to(dev), layer_idx=li)
        assert isinstance(got, np.ndarray) and got.dtype == np.float32
        w = int((S - 1) ** 0.5)
        assert got.shape == ((B, w, w) if kind == "vit" else (B, S - 1))
        one = ro(x[:1].to(dev), layer_idx=li)
        assert one.shape == got.shape[1:] and np.array_equal(one, got[0])          # one input: no batch axis; a batch is B single calls
        ro.remove_hooks()
        mask, zero, fused = device_pipeline([recorded[l] for l in layers], B, S, heads, fusion, ratio, dev)
        assert np.array_equal(mask, got.reshape(B, -1))                          # the classes are the device forms on the recorded qkv
        k = RR.discard_count(S, ratio)
        for b in range(B):
            f64 = [RR.fused_maps(recorded[l].view(B, S, -1)[b].reshape(S, -1), 1, S, heads, fusion)[0] for l in layers]
            f32 = [RR.fused_maps(recorded[l].view(B, S, -1)[b].reshape(S, -1), 1, S, heads, fusion, torch.float32)[0] for l in layers]
            pats = []
            for j in range(len(layers)):
                tau = RR.GATE * RR.rel_err(f32[j], f64[j])
                assert RR.rel_err(fused[j, b], f64[j]) <= tau
                if k:
                    check_band(f64[j], zero[j, b], k, tau, None)
                pats.append(zero[j, b] if k else np.zeros_like(zero[j, b]))
            m64 = RR.rollout64(f64, ratio, pats)
            emu, err = RR.abs_err(RR.rollout32(f32, ratio, pats), m64), RR.abs_err(mask[b], m64)
            print(f"tower {kind} layer_idx={li} ratio={ratio} b={b}: device {err:.3e}, emulation {emu:.3e}, ratio {err / emu:.2f}")
            assert err <= RR.GATE * emu
        if ratio == 0.0:
            o32, o16 = _oracle_masks(O, om, x, layers, heads, fusion, monkeypatch)
            gate = RR.GATE * float(np.abs(o32 - o16).max())
            err = float(np.abs(mask - o32).max())
            print(f"tower {kind}: device vs the oracle's fp32 mask {err:.3e}, oracle bf16 vs fp32 {gate / RR.GATE:.3e}")
            assert err <= gate


def test_vit_tower_end_to_end(dev, monkeypatch):
    from clibd_amd.model.image_encoder import CLIBDImageEncoder, create_vit
    from oracle import clibd_oracle as O

    torch.manual_seed(41)
    om = O.ImageEncoder(O.VisionTransformer(img_size=224, patch=16, dim=128, depth=12, heads=2, num_classes=0), 4, 64)
    _peaky(om)
    m = CLIBDImageEncoder(create_vit("vit_base_patch16_224", num_classes=0, embed_dim=128, depth=12, num_heads=2), r=4, num_classes=64)
    m.load_state_dict(om.state_dict(), strict=True)
    m = m.to(dev).eval()
    x = torch.rand(2, 3, 224, 224, generator=torch.Generator().manual_seed(42))
    _tower_case(dev, m, om.eval(), O, x, "vit", 2, "max", monkeypatch)


def test_barcodebert_tower_end_to_end(dev, monkeypatch):
    from clibd_amd.model.dna_encoder import BertConfigLite, BertForMaskedLM, CLIBDDNAEncoder
    from oracle import clibd_oracle as O

    torch.manual_seed(43)
    om = O.DNAEncoder(O.BertForMaskedLM(vocab=1027, hidden=128, layers=4, heads=2, ff=512), 4, 64)
    _peaky(om)
    m = CLIBDDNAEncoder(BertForMaskedLM(BertConfigLite(vocab_size=1027, hidden_size=128, num_hidden_layers=4, num_attention_heads=2,
                                                      intermediate_size=512)), r=4, num_classes=64)
    m.load_state_dict(om.state_dict(), strict=True)
    m = m.to(dev).eval()
    ids = torch.randint(0, 1027, (2, 133), generator=torch.Generator().manual_seed(44))
    _tower_case(dev, m, om.eval(), O, ids, "dna", 2, "min", monkeypatch)
