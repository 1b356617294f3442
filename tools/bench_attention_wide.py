"""Attention for 128- / 192-wide heads against the 64-wide kernels at the same hidden width, and one LoRA training step of the DNA towers they serve.

    python tools/bench_attention_wide.py [--batch 256] [--seq 133] [--rounds 3] [--out profiles/attention_wide.log]

Kernels: B = 256, S = 133, H = 768 as 12 x 64 (csrc/attention.hip: the yardstick), 6 x 128 and 4 x 192 (csrc/attention_wide.hip), with dropout
p = 0.1 (what a training step runs) and without.  The three splits have identical matrix FLOPs (4 B S^2 H forward, 10 B S^2 H two-phase backward) and
operand bytes; wide heads evaluate fewer exponentials (B heads S^2).  Times are device events around 50 launches after 5 warm-up launches, the forms
alternating inside every round; the spread over the rounds is printed.  Tower step: forward + backward of a CLIBDDNAEncoder (rank-4 LoRA, train
mode, vocabulary 258) at 6 layers / 6 heads and 4 layers / 4 heads, beside 6 layers / 12 heads as the 64-wide control, batch 256.
A machine without a GPU cannot run this (no fallback)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clibd_amd import ops  # noqa: E402

BF16 = torch.bfloat16
H = 768


def timeit(fn, iters=50, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3        # us per launch


def kernel_forms(dev, B, S, nh, p):
    """{name: launch} for one split of H = 768 into nh heads"""
    dh = H // nh
    g = torch.Generator(device=dev).manual_seed(nh)
    qkv = (torch.randn(B * S, 3 * H, device=dev, generator=g) * 0.5).to(BF16)
    do = torch.randn(B * S, H, device=dev, generator=g).to(BF16)
    out, o_lo, dqkv = torch.empty(B * S, H, device=dev, dtype=BF16), torch.empty(B * S, H, device=dev, dtype=BF16), torch.empty_like(qkv)
    lse = torch.empty(B * nh * S, device=dev)
    drop = ops.Drop(p, 5) if p > 0 else None
    if dh == 64:
        ops.attention_fwd(qkv, B, S, nh, None, out, drop=drop, lse=lse, o_lo=o_lo)
        return {"fwd": lambda: ops.attention_fwd(qkv, B, S, nh, None, out, drop=drop),
                "fwd+lse": lambda: ops.attention_fwd(qkv, B, S, nh, None, out, drop=drop, lse=lse, o_lo=o_lo),
                "bwd": lambda: ops.attention_bwd(qkv, do, B, S, nh, None, dqkv, drop=drop),
                "bwd single-pass": lambda: ops.attention_bwd_sp(qkv, do, out, o_lo, lse, B, S, nh, dqkv, drop=drop)}
    ops.attention_wide_fwd(qkv, B, S, nh, dh, out, lse=lse, drop=drop)
    return {"fwd": lambda: ops.attention_wide_fwd(qkv, B, S, nh, dh, out, drop=drop),
            "fwd+lse": lambda: ops.attention_wide_fwd(qkv, B, S, nh, dh, out, lse=lse, drop=drop),
            "bwd": lambda: ops.attention_wide_bwd(qkv, do, lse, B, S, nh, dh, dqkv, drop=drop)}


def tower_step(dev, layers, heads, B, S):
    from clibd_amd.model import BertConfigLite, BertForMaskedLM, CLIBDDNAEncoder

    torch.manual_seed(layers)
    m = CLIBDDNAEncoder(BertForMaskedLM(BertConfigLite(vocab_size=258, hidden_size=H, num_hidden_layers=layers, num_attention_heads=heads,
                                                       intermediate_size=4 * H)), r=4, num_classes=H).to(dev).train()
    with torch.no_grad():
        for w in m.w_Bs:
            w.weight.normal_(0, 0.02)
    ids = torch.cat([torch.zeros(B, 1, dtype=torch.long), torch.randint(2, 258, (B, S - 1))], dim=1).to(dev)
    cot = torch.randn(B, H, device=dev)
    ps = [p for p in m.parameters() if p.requires_grad]

    def step():
        torch.autograd.grad((m(ids) * cot).sum(), ps)

    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--seq", type=int, default=133)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "attention_wide.log"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attention_wide: needs an MI355X (timings are GPU measurements; there is no fallback)")
    dev = torch.device("cuda:0")
    B, S = a.batch, a.seq
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    from clibd_amd.build import csrc_hash

    say(f"# tools/bench_attention_wide.py  B={B} S={S} H={H}  csrc {csrc_hash()}  {torch.cuda.get_device_name(0)}  us per launch: median [min .. max] of {a.rounds} rounds x 50 launches")
    say(f"# matrix FLOPs per launch: forward {4 * B * S * S * H / 1e9:.1f} G, two-phase backward {10 * B * S * S * H / 1e9:.1f} G; operand bytes: qkv {B * S * 3 * H * 2 / 1e6:.0f} MB")
    med = {}
    for p in (0.1, 0.0):
        forms = {nh: kernel_forms(dev, B, S, nh, p) for nh in (12, 6, 4)}
        times = {(nh, k): [] for nh, f in forms.items() for k in f}
        for _ in range(a.rounds):
            for k in ("fwd", "fwd+lse", "bwd", "bwd single-pass"):
                for nh in (12, 6, 4):
                    if k in forms[nh]:
                        times[(nh, k)].append(timeit(forms[nh][k]))
        for (nh, k), t in times.items():
            t = sorted(t)
            med[(p, nh, k)] = t[len(t) // 2]
            say(f"p={p}  {nh:2d} x {H // nh:3d}  {k:16s} {t[len(t) // 2]:8.1f}  [{t[0]:8.1f} .. {t[-1]:8.1f}]")
        for nh in (6, 4):
            say(f"p={p}  ratio to 12 x 64:  {nh} x {H // nh}  fwd {med[(p, nh, 'fwd')] / med[(p, 12, 'fwd')]:.2f}  fwd+lse {med[(p, nh, 'fwd+lse')] / med[(p, 12, 'fwd+lse')]:.2f}  "
                f"bwd / two-phase {med[(p, nh, 'bwd')] / med[(p, 12, 'bwd')]:.2f}  bwd / single-pass {med[(p, nh, 'bwd')] / med[(p, 12, 'bwd single-pass')]:.2f}")
        del forms
    steps = {(L, nh): tower_step(dev, L, nh, B, S) for L, nh in ((6, 12), (6, 6), (4, 4))}
    ts = {k: [] for k in steps}
    for _ in range(a.rounds):
        for k, fn in steps.items():
            ts[k].append(timeit(fn, iters=10, warm=2) / 1e3)
    for (L, nh), t in ts.items():
        t = sorted(t)
        say(f"DNA tower LoRA step (forward + backward, train mode)  {L} layers x {nh:2d} heads (head_dim {H // nh:3d})  b={B}: {t[len(t) // 2]:7.2f} ms  [{t[0]:7.2f} .. {t[-1]:7.2f}]")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
