"""The chunked contrastive step: the exact full-batch contrastive gradient with the activations of one chunk in memory.

A contrastive loss couples every row of the batch with every other one, so the loss of k micro-batches is not the loss of the batch k times
the size and gradient accumulation (clibd_amd.optim, §3.18) does not apply.  What does factor is the chain rule at the embeddings
(GradCache, Gao et al. 2021): the towers are row-independent, the loss needs the b embeddings only, and a tower's backward over the batch is
the sum of its backwards over row ranges.  `two_pass` is that schedule, shared by `train.Trainer(chunk_size=...)` and
`simclr.SimCLR(chunk_size=...)`:

  pass 1  every chunk runs forward under torch.no_grad() in the model's current train / eval mode; its embeddings go into an fp32 [b, D]
          cache per output.  The CPU generator's state is recorded before each chunk's forward (the towers draw their dropout base there).
  root    the criterion runs ONCE on the caches as leaf tensors, all b rows, the real logit_scale; loss.backward() leaves dE for every
          cached row in the leaves' .grad and the temperature gradient where it belongs.  Under data-parallel training this is the step's
          one all-gather and one reduce-scatter.
  pass 2  chunk by chunk: the recorded generator state is restored, the forward runs again with saving, and ONE torch.autograd.backward
          call takes all of the chunk's embeddings with their rows of dE (the towers' backwards overlap on their streams as in the plain
          step).  Parameter gradients accumulate (flat bucket or .grad); the chunk's saved state is gone before the next chunk's forward.
          After the last chunk the generator is put into the state pass 1 left it in.

The replay rule: pass 2 must reproduce pass 1's embeddings bit for bit, otherwise dE belongs to other embeddings than the ones it is pushed
through.  Two things make it so.  The generator restore gives each chunk the dropout base it had in pass 1 (a fresh base per chunk, row
indices local to the chunk: chunked and unchunked masks differ by design).  And pass 1 runs the training forward's arithmetic
(`TransformerStack.train_arithmetic`): the plain no-grad forward applies GELU to the fp32 pre-activation, the saving forward to its bf16
rounding.  `ReplayGuard` counts, on the device and without a host synchronisation, the cached words pass 2 failed to reproduce.

No arithmetic of its own: every launch is an existing HIP kernel; torch supplies views, row slices, the cache copies and the guard's compare.
"""
from __future__ import annotations

import contextlib
from typing import Callable, List, Optional, Sequence, Tuple

import torch

F32 = torch.float32


def validate_chunk_size(chunk_size, who: str) -> Optional[int]:
    """None (the plain step) or an integer >= 1 (samples per chunk); anything else raises ValueError"""
    if chunk_size is None:
        return None
    if isinstance(chunk_size, bool) or not isinstance(chunk_size, int) or chunk_size < 1:
        raise ValueError(f"{who}: chunk_size must be None or an integer >= 1 (samples per chunk), got {chunk_size!r}")
    return chunk_size


def plan_chunks(b: int, chunk_size: int) -> List[Tuple[int, int]]:
    """[(lo, hi)] row ranges covering 0..b in order, each chunk_size long except a shorter last one; chunk_size >= b is one chunk"""
    validate_chunk_size(chunk_size, "plan_chunks")
    if isinstance(b, bool) or not isinstance(b, int) or b < 1:
        raise ValueError(f"plan_chunks: the batch must hold at least one row, got {b!r}")
    return [(lo, min(lo + chunk_size, b)) for lo in range(0, b, chunk_size)]


def slice_rows(x, lo: int, hi: int):
    """rows lo..hi of a model input as views: a tensor, a dict of tensors (the text input), a tuple / list of those, or None"""
    if x is None:
        return None
    if torch.is_tensor(x):
        return x[lo:hi]
    if isinstance(x, dict):
        return {k: slice_rows(v, lo, hi) for k, v in x.items()}
    if isinstance(x, (tuple, list)):
        return type(x)(slice_rows(v, lo, hi) for v in x)
    raise TypeError(f"chunked step: cannot slice an input of type {type(x).__name__}")


def batch_rows(x) -> int:
    """the number of rows of the first tensor found in an input (see slice_rows)"""
    if torch.is_tensor(x):
        return int(x.shape[0])
    if isinstance(x, dict):
        x = list(x.values())
    if isinstance(x, (tuple, list)):
        for v in x:
            if v is not None:
                return batch_rows(v)
    raise ValueError("chunked step: no input tensor to take the batch size from")


class ReplayGuard:
    """`mismatch`: device int64 [1], the number of cached embedding words (fp32 words compared as bits, so NaN equals itself and -0 differs
    from +0) that pass 2 did not reproduce, summed over every chunked step since construction.  Nothing here reads it back."""

    def __init__(self, device):
        self.mismatch = torch.zeros((1,), dtype=torch.int64, device=device)

    def check(self, out: torch.Tensor, cached: torch.Tensor) -> None:
        self.mismatch += (out.detach().view(torch.int32) != cached.detach().view(torch.int32)).sum()


@contextlib.contextmanager
def _training_arithmetic(towers):
    """pass 1: the towers' stacks evaluate the saving forward's expressions although nothing is saved (engine.TransformerStack)"""
    stacks = [tw.stack for tw in towers if hasattr(tw, "stack")]
    before = [st.train_arithmetic for st in stacks]
    for st in stacks:
        st.train_arithmetic = True
    try:
        yield
    finally:
        for st, was in zip(stacks, before):
            st.train_arithmetic = was


@contextlib.contextmanager
def _hooks_inert(towers):
    """every chunk but the last: gradients in the bucket are partial sums, so the towers' gradient-ready hooks (the trainer's bucketed
    all-reduce) must not fire"""
    before = [tw.__dict__.get("on_grads_ready", _ABSENT) for tw in towers]
    for tw in towers:
        tw.on_grads_ready = None
    try:
        yield
    finally:
        for tw, was in zip(towers, before):
            if was is _ABSENT:
                del tw.on_grads_ready
            else:
                tw.on_grads_ready = was


_ABSENT = object()


def two_pass(forward: Callable, inputs: Sequence, chunk_size: int, root_loss: Callable, towers: Sequence = (), side_streams: Sequence = (),
             join: Optional[Callable] = None, guard: Optional[ReplayGuard] = None, generator_state=(torch.get_rng_state, torch.set_rng_state)):
    """forward(*chunk inputs) -> tuple of [rows, D] embeddings (None for an absent modality); inputs: the whole batch, one entry per argument
    of `forward` (tensor, dict of tensors or None), sliced by row as views; root_loss(leaves) -> scalar loss over all b rows, `leaves` being the
    fp32 caches as leaf tensors in `forward`'s output order.  towers: the model's towers (arithmetic switch of pass 1, hooks inert until the
    last chunk).  side_streams / join: the streams the towers run on besides the current one (a list, or a callable returning it), and the call that makes the current stream wait
    for them (SimpleCLIP.join_streams).  Returns (detached loss, caches).  Parameter gradients have been accumulated; on return the current
    stream is ordered after every tower's backward and the CPU generator is in the state pass 1 left."""
    get_state, set_state = generator_state
    plan = plan_chunks(batch_rows(list(inputs)), chunk_size)
    b = plan[-1][1]
    states, caches = [], None
    # ---- pass 1: embeddings of every chunk, nothing saved
    with torch.no_grad(), _training_arithmetic(towers):
        for lo, hi in plan:
            states.append(get_state())
            outs = forward(*[slice_rows(x, lo, hi) for x in inputs])
            if caches is None:
                caches = [None if o is None else torch.empty((b, o.shape[1]), dtype=F32, device=o.device) for o in outs]
            for c, o in zip(caches, outs):
                if c is not None:
                    c[lo:hi].copy_(o)      # on the current stream: `forward` returns outputs the current stream may read (it has waited for their streams)
            del outs
    end_state = get_state()
    # ---- the loss at the root: all b rows, once
    leaves = [None if c is None else c.requires_grad_(True) for c in caches]
    loss = root_loss(leaves)
    loss.backward()
    d_emb = [None if c is None else c.grad for c in leaves]
    if callable(side_streams):
        side_streams = side_streams()      # asked for now: a model creates its streams in its first forward
    if side_streams:
        main = torch.cuda.current_stream(next(c for c in caches if c is not None).device)
        for st in side_streams:
            st.wait_stream(main)           # dE was produced on the current stream; the towers' backwards read it on theirs
            for g in d_emb:
                if g is not None:
                    g.record_stream(st)
    # ---- pass 2: replay each chunk with saving and push its rows of dE through it
    for i, (lo, hi) in enumerate(plan):
        set_state(states[i])
        with (contextlib.nullcontext() if i == len(plan) - 1 else _hooks_inert(towers)):
            outs = forward(*[slice_rows(x, lo, hi) for x in inputs])
            if guard is not None:
                for c, o in zip(caches, outs):
                    if c is not None:
                        guard.check(o, c[lo:hi])
            live = [(o, g[lo:hi]) for o, g in zip(outs, d_emb) if o is not None and o.requires_grad]
            if live:
                torch.autograd.backward([o for o, _ in live], [g for _, g in live])
        del outs, live                      # the chunk's graph and saved activations go before the next chunk's forward
    set_state(end_state)
    if join is not None:
        join()
    for c in leaves:
        if c is not None:
            c.grad = None
            c.requires_grad_(False)
    return loss.detach(), caches
