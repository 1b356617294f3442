"""Generate tests/golden/simclr_golden.pt from the reference's own SimCLR.info_nce_loss + CrossEntropyLoss (authoring box only).

    python tools/make_simclr_golden.py --reference <checkout of the reference>

The reference's bioscanclip/util/simclr.py is imported with empty stub modules for wandb, torch.utils.tensorboard, tqdm and yaml where
they are absent (the SURVEY §8c technique) and evaluated in fp32 on the CPU.  Only data is written: per case the seeded inputs, the
loss and d loss / d features.  No test on the GPU and no smoke run reads the reference; tests/test_simclr_cpu.py checks its own fp64
restatement of the loss against this file.
"""
import argparse
import importlib
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(4, 1000, 101), (16, 768, 102)]   # (b, D, seed)
TEMPERATURE = 0.07


def _stub(name, **attrs):
    try:
        return importlib.import_module(name)
    except Exception:
        m = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m
        parent, _, child = name.rpartition(".")
        if parent and parent in sys.modules:
            setattr(sys.modules[parent], child, m)
        return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout (the directory that holds bioscanclip/)")
    a = ap.parse_args()
    _stub("wandb")
    _stub("torch.utils.tensorboard", SummaryWriter=object)
    _stub("tqdm", tqdm=lambda it, *x, **k: it)
    _stub("yaml")
    sys.path.insert(0, a.reference)
    spec = importlib.util.spec_from_file_location("ref_simclr", os.path.join(a.reference, "bioscanclip", "util", "simclr.py"))
    R = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(R)

    out = {"temperature": TEMPERATURE, "cases": []}
    for b, D, seed in CASES:
        sim = object.__new__(R.SimCLR)      # its __init__ opens a tensorboard writer and creates directories: not needed for the loss
        sim.args = types.SimpleNamespace(model_config=types.SimpleNamespace(batch_size=b, n_views=2, temperature=TEMPERATURE))
        sim.device = torch.device("cpu")
        f = (torch.randn(2 * b, D, generator=torch.Generator().manual_seed(seed)) * 3).requires_grad_(True)
        logits, labels = sim.info_nce_loss(f)
        loss = torch.nn.CrossEntropyLoss()(logits, labels)
        (df,) = torch.autograd.grad(loss, f)
        top1 = int((logits.argmax(dim=1) == labels).sum())
        out["cases"].append({"b": b, "D": D, "seed": seed, "features": f.detach().clone(), "loss": loss.detach().clone(), "dfeatures": df.clone(),
                             "top1_hits": top1})
        print(f"b={b} D={D}: loss {loss.item():.6f}, |df| {df.norm().item():.4e}, top-1 hits {top1}/{2 * b}")
    path = os.path.join(ROOT, "tests", "golden", "simclr_golden.pt")
    torch.save(out, path)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
