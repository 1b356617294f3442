"""What one training / eval step of the towers enqueues, configuration by configuration: every C-ABI call with its scalar arguments, the
fields of its epilogue struct and the NULL pattern of its pointers, then a sha256 of every tower output and parameter gradient and the
step's peak device memory.  Two trees that print the same text launch the same kernels on the same operands and compute the same bits:
the acceptance check of a host-side restructuring of clibd_amd/engine.py (run it on both trees, `diff` the outputs).

usage: python tools/stack_plan.py [--tree DIR] [--digest FILE] [--coverage] > plan.txt
  --digest FILE  also write the plan's short form to FILE (what profiles/ keeps: the full text is half a megabyte): per configuration
               the number of calls and a sha256 over their lines, the calls per symbol, the tower outputs' hashes, a sha256 over the
               gradients' hash lines, the peak bytes.  Equal digests = equal plans; where two differ, diff the full texts
  --tree DIR   import clibd_amd from DIR instead of this checkout (a second tree beside this one; CLIBD_HIP_LIB names its library)
  --coverage   run the same matrix under sys.settrace and list the `ops.` lines of TransformerStack's step code no configuration reached
               (the matrix is only an argument for the whole of that code if the list is empty)
Line format: symbol, then the arguments in order — integers and floats by value, pointers as p (0 = NULL), the epilogue struct as
{pointer fields as p/0 | the scalar fields}.  The towers run on one stream (CLIBD_TOWER_STREAMS=0) so that the order is the program's."""
import ctypes, gc, hashlib, inspect, os, sys

os.environ.setdefault("CLIBD_TOWER_STREAMS", "0")
ARGS = sys.argv[1:]
TREE = ARGS[ARGS.index("--tree") + 1] if "--tree" in ARGS else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.abspath(TREE))
import torch
from clibd_amd import _lib, engine
from clibd_amd.data import synthetic_batch
from clibd_amd.model import (BertConfigLite, BertForMaskedLM, BertModel, CLIBDDNAEncoder, CLIBDImageEncoder, CLIBDLanguageEncoder, ClipLoss,
                             SimpleCLIP, create_vit)
from clibd_amd.model.dna_encoder import kmer_vocab
from clibd_amd.model.language_encoder import BERT_SMALL

DEV = torch.device("cuda:0")
SIGS = _lib.SIGNATURES


def _scalar(ctype, v):
    if ctype is ctypes.c_void_p or ctype is ctypes.c_char_p:
        return "0" if not v else "p"
    return repr(float(ctypes.c_float(v).value)) if ctype in (ctypes.c_float, ctypes.c_double) else str(int(v))


def _struct(ep):
    ptrs = "".join(_scalar(t, getattr(ep, n)) for n, t in ep._fields_ if t is ctypes.c_void_p)
    return "{" + ptrs + "|" + ",".join(_scalar(t, getattr(ep, n)) for n, t in ep._fields_ if t is not ctypes.c_void_p) + "}"


class Recorder:
    """stands in for the loaded library: prints every clibd_* launch (not the *_workspace_bytes / error / version queries) as it is made"""

    def __init__(self, lib):
        self._lib, self.on = lib, False

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("clibd_") or not callable(fn) or name.endswith("_bytes") or SIGS[name][0] is not ctypes.c_int or not SIGS[name][1]:
            return fn
        types = SIGS[name][1]

        def wrapped(*args):
            if self.on:
                print(name[6:], *(_struct(a._obj) if hasattr(a, "_obj") else _scalar(t, a) for t, a in zip(types, args)), flush=True)
            return fn(*args)

        return wrapped


def build(text=True, r=4, top_only=False, full=False):
    """depth 2 at full width: ViT-B/16 blocks (the second one runs class-row-only), BarcodeBERT layers, BERT-small layers"""
    torch.manual_seed(11)
    ll = [1] if top_only else None
    model = SimpleCLIP(CLIBDImageEncoder(create_vit("vit_base_patch16_224", depth=2), r=r, num_classes=768, lora_layer=ll),
                       CLIBDDNAEncoder(BertForMaskedLM(BertConfigLite(vocab_size=len(kmer_vocab(5)), num_hidden_layers=2)), r=r, num_classes=768,
                                       lora_layer=ll),
                       CLIBDLanguageEncoder(BertModel(BertConfigLite(**dict(BERT_SMALL, num_hidden_layers=2))), r=r, num_classes=768,
                                            lora_layer=ll) if text else None)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "linear_b_" in n or ".w_b." in n:
                p.normal_(0, 0.02)
    if full:
        for p in model.parameters():
            p.requires_grad_(True)
    return model.to(DEV)


def run(rec, tag, model, B=8, train=False, grad=True, det=True, hashes=True):
    """one step of `model` (forward, loss, backward — or the forward alone under no_grad): trace, hashes, peak bytes"""
    batch = synthetic_batch(B, DEV, seed=7, rank=0, with_text=model.language_encoder is not None)
    model.train(train)
    model.set_deterministic(det)
    torch.manual_seed(123)   # the towers draw their dropout base seeds from the CPU generator
    # the peak is to be a property of the step's own allocations: no cached blocks of earlier configurations to reuse unsplit, and no
    # cycle collection in the middle of the step (its moment depends on how many Python objects the host code happened to create)
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    gc.disable()
    print(f"==== {tag}: B={B} {'train' if train else 'eval'} mode, {'step' if grad else 'no_grad'}, deterministic={det}", flush=True)
    rec.on = True
    named = []
    if grad:
        ps = {n: p for n, p in model.named_parameters() if p.requires_grad}
        crit = ClipLoss(local_loss=False, gather_with_grad=True, rank=0, world_size=1, criterion=torch.nn.CrossEntropyLoss())
        hi, hd, ht, scale, _ = model(batch["image"], batch["dna"], batch["text"])
        gs = torch.autograd.grad(crit(hi, hd, ht, batch["labels"], scale), list(ps.values()), allow_unused=True)
        named = [(n, g) for n, g in zip(ps, gs) if g is not None]
    else:
        with torch.no_grad():
            hi, hd, ht, _, _ = model(batch["image"], batch["dna"], batch["text"])
    model.join_streams()
    torch.cuda.synchronize()
    gc.enable()
    rec.on = False
    if hashes:
        for n, t in [("out.image", hi), ("out.dna", hd), ("out.text", ht)] + named:
            if t is not None:
                print("sha256", n, hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()[:32])
    print("peak_bytes", torch.cuda.max_memory_allocated(), flush=True)
    del hi, hd, ht, named


def matrix(rec):
    """the configurations (1-8: LoRA, 9: full fine-tune); each `model` is dropped before the next is built"""
    m = build()
    run(rec, "1 lora r4 trimodal", m, train=True)
    run(rec, "1 lora r4 trimodal", m, grad=False)
    m.set_numerics(residual_grad="fp32"); run(rec, "2 residual_grad=fp32", m, train=True); m.set_numerics(residual_grad="bf16")
    for gg in ("u8", "e4m7"):
        m.set_numerics(gelu_grad=gg); run(rec, f"3 gelu_grad={gg}", m)
    m.set_numerics(gelu_grad="bf16", attn_bwd="sp"); run(rec, "4 attn_bwd=sp", m, train=True); m.set_numerics(attn_bwd="2phase")
    for sites in (("mlp",), ("proj",), ("mlp", "proj")):
        m.set_numerics(dgrad="fp8")
        for st in m._stacks():
            st.dgrad8_sites = sites
        run(rec, f"8 dgrad=fp8 sites={'+'.join(sites)}", m, train=len(sites) == 2)
    run(rec, "8 dgrad=fp8, token count no multiple of 4", m, B=5)
    m.set_numerics(dgrad="bf16")
    cal = synthetic_batch(8, DEV, seed=9, rank=0, with_text=True)
    for towers in ("all", "pooled_ffn", "pooled_mlp"):   # (pooled_mlp: the ViT's MLP pair — the pre-LN form of the site selection)
        print(f"==== 7 fp8 forward {towers}: calibration pass", flush=True)
        rec.on = True
        m.eval().enable_fp8_forward(towers=towers, calibration_inputs=(cal["image"], cal["dna"], cal["text"]))
        rec.on = False
        run(rec, f"7 fp8 forward {towers}", m, train=True)
        run(rec, f"7 fp8 forward {towers}", m, grad=False)
    del m
    m = build(text=False).set_numerics(ln_fold="on")
    run(rec, "5 ln_fold=on", m, B=64)
    run(rec, "5 ln_fold=on", m, B=64, grad=False)
    for r in (2, 6):
        del m
        m = build(r=r, top_only=True)
        run(rec, f"6 lora r{r}, top layer only", m, train=True)
    del m
    m = build(r=6)   # (every layer: the second slot's addend joins the QKV dgrad of the backward, which the top-only models stop short of)
    run(rec, "6 lora r6, every layer", m, train=True)
    del m
    m = build(text=False, full=True)
    run(rec, "9 full fine-tune bf16", m, train=True)
    run(rec, "9 full fine-tune bf16 (trace only)", m, train=True, det=False, hashes=False)
    m.set_numerics(residual_grad="fp32"); run(rec, "9 full fine-tune residual_grad=fp32", m, train=True); m.set_numerics(residual_grad="bf16")
    m.enable_fp8_dgrad("all"); run(rec, "9 full fine-tune dgrad=fp8", m, train=True); m.enable_fp8_dgrad("all", enabled=False)
    for vit in (False, True):   # pooled_ffn: the MLP pair of the mean-pooled tower; then the ViT's MLP pair with it (the pre-LN form)
        m.enable_fp8_forward(towers="pooled_ffn")
        if vit:
            m.image_encoder.tower().stack.enable_fp8(sites=("fc1_in", "fc2_in"))
        tag = "9 full fine-tune fp8 forward pooled_ffn" + (" + ViT MLP pair" if vit else "")
        run(rec, tag, m, train=True)
        m.enable_fp8_dgrad("all"); run(rec, tag + " + dgrad=fp8", m, train=True); m.enable_fp8_dgrad("all", enabled=False)
    m.enable_fp8_forward(enabled=False)


STEP_CODE_EXCLUDES = ("__init__", "set_numerics", "_dgrad8_ok", "enable_fp8", "disable_fp8", "calibrate", "_key", "full_mode", "base_params", "refresh",
                      "pack_lora", "lora_a", "layer_params")   # set-up code: everything else of TransformerStack is what a step runs


def _code_lines(code):
    """the lines of a function that hold instructions (docstrings and comments do not), nested lambdas / functions included"""
    lines = {ln for _, _, ln in code.co_lines() if ln is not None}
    for c in code.co_consts:
        if inspect.iscode(c):
            lines |= _code_lines(c)
    return lines


class Tee:
    """stdout that also keeps what passes through (the trace still leaves line by line: after a fault the last line names the call)"""

    def __init__(self, out):
        self.out, self.text = out, []

    def write(self, t):
        self.text.append(t)
        return self.out.write(t)

    def flush(self):
        self.out.flush()


def digest(text):
    sha = lambda ls: hashlib.sha256("\n".join(ls).encode()).hexdigest()[:32]
    head, *blocks = text.split("==== ")
    out = [head.strip()]
    for b in blocks:
        tag, *ls = b.strip().split("\n")
        calls = [l for l in ls if not l.startswith(("sha256 ", "peak_bytes "))]
        grads = [l for l in ls if l.startswith("sha256 ") and not l.startswith("sha256 out.")]
        count = {}
        for l in calls:
            count[l.split()[0]] = count.get(l.split()[0], 0) + 1
        out += ["==== " + tag, f"calls {len(calls)} sha256 {sha(calls)}", "  " + " ".join(f"{k}={v}" for k, v in sorted(count.items()))]
        out += [l for l in ls if l.startswith("sha256 out.")] + ([f"gradients {len(grads)} sha256 {sha(grads)}"] if grads else [])
        out += [l for l in ls if l.startswith("peak_bytes ")]
    return "\n".join(out) + "\n"


def main():
    if "--digest" in ARGS:
        sys.stdout = tee = Tee(sys.stdout)
        try:
            return _main()
        finally:
            sys.stdout = tee.out
            with open(ARGS[ARGS.index("--digest") + 1], "w") as f:
                f.write(digest("".join(tee.text)))
    return _main()


def _main():
    real = _lib.load()
    rec = Recorder(real)
    _lib.load = lambda: rec
    print("build_hash", (real.clibd_build_hash() or b"").decode(), file=sys.stderr if "--coverage" in ARGS else sys.stdout)
    print("tree", os.path.dirname(engine.__file__), file=sys.stderr)
    if "--coverage" not in ARGS:
        return matrix(rec)
    want, seen, codes = {}, set(), set()
    for name, fn in vars(engine.TransformerStack).items():
        if inspect.isfunction(fn) and name not in STEP_CODE_EXCLUDES:
            src, first = inspect.getsourcelines(fn)
            want.update({first + k: (name, s.strip()) for k, s in enumerate(src) if "ops." in s and first + k in _code_lines(fn.__code__)})
            codes.add(fn.__code__.co_filename)

    def tracer(frame, event, arg):   # (nested lambdas and helpers of engine.py included: the file decides)
        if frame.f_code.co_filename not in codes:
            return None
        seen.add(frame.f_lineno)
        return tracer

    for name in ("forward", "backward"):   # the backward runs on autograd's thread: the trace function is set where the method is entered
        def traced(self, *a, __orig=getattr(engine.TransformerStack, name), **k):
            sys.settrace(tracer)
            try:
                return __orig(self, *a, **k)
            finally:
                sys.settrace(None)
        setattr(engine.TransformerStack, name, traced)
    with open(os.devnull, "w") as null:
        out, sys.stdout = sys.stdout, null
        try:
            matrix(rec)
        finally:
            sys.stdout = out
    missed = sorted(set(want) - seen)
    print(f"{len(want)} `ops.` lines in TransformerStack's step code, {len(missed)} never executed")
    for ln in missed:
        print(f"  engine.py:{ln} ({want[ln][0]}): {want[ln][1]}")


if __name__ == "__main__":
    main()
