"""Generate tests/golden/rollout_golden.pt: what the reference's own `rollout` functions return
(scripts/result/representation_visualization/image_representation_visualization.py and dna_representation_visualization.py) on synthetic
attentions (authoring container only).

    python tests/golden/make_rollout_golden.py       # needs /root/reference; writes tests/golden/rollout_golden.pt

The two scripts are imported under the stub pattern of make_method_linear_golden.py: cv2, h5py, hydra, omegaconf, torchvision, matplotlib and
the bioscanclip modules they import are empty stand-ins (their `rollout` needs torch and numpy only).  Only data is written: masks, seeds,
measured gaps and, for (B), the bit-packed index sets of the reference's torch.topk.  Inputs are regenerated from seeds on both sides
(tests/rollout_reference.py: synth_qkv, synth_maps).

(A) from qkv: S = 17, 3 heads, 12 layers, qkv of layer l = synth_qkv([seed, l], 1, 17, 3).  The reference receives the fp64 probabilities
    rounded once to fp32 as its hooked [1, 3, 17, 17] attentions.  Recorded: its mask for every (script, fusion, ratio, layer_idx) of
    {vit, dna} x {mean, max, min} x {0.9, 0} x {None, 3} (the ViT's reshaped to 4 x 4).  Asserted: at every map's boundary the relative gap
    from the k-th to the (k + 1)-th smallest entry is >= 64 x the fp32 emulation's error on that map, and row 0 of layer 3 keeps at least
    two entries beside [0, 0] under every fusion at ratio 0.9 (a single-layer mask is that row: with none left the reference returns 0/0).
    The seed is the first that passes both.
(B) single-head attentions handed over as maps: S = 197 and S = 133, 12 layers, fp32 maps = synth_maps(seed, 12, S), ratio 0.9, through the
    ViT script (window [1:-6], 14 x 14) and the DNA script (window [1:]).  Asserted: no tie at any boundary, and the reference's topk index
    set equals the stated rule's on every map.
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.dirname(HERE))
import rollout_reference as RR  # noqa: E402

A_CFG = dict(S=17, heads=3, layers=12, ratios=[0.9, 0.0], layer_idx=[None, 3], fusions=["mean", "max", "min"])
B_CFG = {"vit": dict(S=197, layers=12, seed=411), "dna": dict(S=133, layers=12, seed=412)}
GAP_FACTOR = 64


def import_reference():
    sys.path.insert(0, HERE)
    import make_golden as MG

    MG.install_stubs()
    MG._stub("cv2")
    MG._stub("h5py")
    MG._stub("hydra", main=lambda *a, **k: (lambda f: f))
    MG._stub("omegaconf", OmegaConf=MG._Anything, DictConfig=dict, open_dict=MG._Anything())
    MG._stub("torchvision", transforms=MG._Anything())
    MG._stub("torchvision.transforms")
    MG._stub("matplotlib")
    MG._stub("matplotlib.pyplot")
    MG._stub("bioscanclip")
    MG._stub("bioscanclip.model")
    MG._stub("bioscanclip.model.simple_clip", load_clip_model=MG._Anything())
    MG._stub("bioscanclip.model.dna_encoder", get_sequence_pipeline=MG._Anything())
    MG._stub("bioscanclip.util")
    MG._stub("bioscanclip.util.util", update_checkpoint_param_names=MG._Anything())
    MG._stub("bioscanclip.util.dataset", tokenize_dna_sequence=MG._Anything())
    out = {}
    for kind, name in (("vit", "image_representation_visualization"), ("dna", "dna_representation_visualization")):
        spec = importlib.util.spec_from_file_location(f"ref_{name}", os.path.join(REF, "scripts", "result", "representation_visualization", f"{name}.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        out[kind] = mod
    return out


def a_inputs(seed: int, cfg=A_CFG):
    """per layer: (P fp64 [1, heads, S, S], P fp32 emulation) of the seeded qkv"""
    import torch

    S, heads = cfg["S"], cfg["heads"]
    p64, p32 = [], []
    for l in range(cfg["layers"]):
        qkv = RR.synth_qkv([seed, l], 1, S, heads)
        p64.append(RR.probs(qkv, 1, S, heads, torch.float64))
        p32.append(RR.probs(qkv, 1, S, heads, torch.float32))
    return p64, p32


def a_gaps(p64, p32, cfg=A_CFG):
    """min over the maps of gap / emulation error, and the extremes"""
    S = cfg["S"]
    worst, gaps, errs = np.inf, [], []
    for fusion in cfg["fusions"]:
        for l in range(cfg["layers"]):
            F64 = RR.fuse(p64[l], fusion)[0].numpy()
            F32 = RR.fuse(p32[l], fusion)[0].numpy()
            err = RR.rel_err(F32, F64)
            for ratio in cfg["ratios"]:
                k = RR.discard_count(S, ratio)
                if k == 0:
                    continue
                _, gap = RR.boundary(F64, k)
                gaps.append(gap)
                errs.append(err)
                worst = min(worst, gap / err)
    return worst, min(gaps), max(gaps), max(errs)


def main():
    import torch

    R = import_reference()
    out = {"A": {"cfg": A_CFG}, "B": {}}

    # ---- (A)
    for seed in range(300, 400):
        p64, p32 = a_inputs(seed)
        worst, gmin, gmax, emax = a_gaps(p64, p32)
        k9 = RR.discard_count(A_CFG["S"], 0.9)
        kept = min(int((~RR.discard_pattern(RR.fuse(p64[3], f)[0].numpy(), k9))[0, 1:].sum()) for f in A_CFG["fusions"])
        if worst >= GAP_FACTOR and kept >= 2:
            break
    else:
        raise RuntimeError("no seed with clear boundaries")
    print(f"(A) seed {seed}: boundary gaps {gmin:.2e} .. {gmax:.2e}, emulation error <= {emax:.2e}, min gap / error {worst:.0f}")
    attn = [p.to(torch.float32) for p in p64]      # what the hook would have handed over: fp32 [1, heads, S, S]
    masks = {}
    for kind in ("vit", "dna"):
        for fusion in A_CFG["fusions"]:
            for ratio in A_CFG["ratios"]:
                for li in A_CFG["layer_idx"]:
                    m = R[kind].rollout([a.clone() for a in attn], ratio, fusion, li)
                    masks[(kind, fusion, ratio, li)] = np.asarray(m, dtype=np.float32).copy()
    assert not any(np.isnan(m).any() for m in masks.values())
    assert masks[("vit", "max", 0.9, None)].shape == (4, 4) and masks[("dna", "max", 0.9, None)].shape == (16,)
    out["A"].update(seed=seed, masks=masks, gap_min=gmin, gap_max=gmax, emu_err_max=emax)

    # ---- (B)
    for kind, cfg in B_CFG.items():
        S, L = cfg["S"], cfg["layers"]
        maps = RR.synth_maps(cfg["seed"], L, S)
        k = RR.discard_count(S, 0.9)
        packed = []
        for l in range(L):
            flat = np.sort(maps[l].reshape(-1))
            assert flat[k - 1] < flat[k], (kind, l)                    # no tie at the boundary, in the fp32 bits both sides see
            _, idx = torch.from_numpy(maps[l].reshape(1, -1).copy()).topk(k, -1, False)     # the reference's own call
            z = np.zeros(S * S, dtype=bool)
            z[idx[0].numpy()] = True
            z[0] = False
            assert np.array_equal(z.reshape(S, S), RR.discard_pattern(maps[l], k)), (kind, l)
            packed.append(np.packbits(z))
        m = R[kind].rollout([torch.from_numpy(maps[l].copy())[None, None] for l in range(L)], 0.9, "max", None)
        m = np.asarray(m, dtype=np.float32).copy()
        assert m.shape == ((14, 14) if kind == "vit" else (S - 1,))
        out["B"][kind] = dict(cfg, ratio=0.9, mask=m, patterns=np.stack(packed))
    path = os.path.join(HERE, "rollout_golden.pt")
    torch.save(out, path)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
