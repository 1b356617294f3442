"""CPU checks of the chunked contrastive step (clibd_amd.chunked): the chunk planner, the validation of chunk_size in both
drivers, and the generator-state record / restore protocol of the two passes on a stub model that draws with torch.randint as the towers do."""
import pytest
import torch

from clibd_amd import chunked


# ---- planner ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,want", [(1, [(i, i + 1) for i in range(8)]), (3, [(0, 3), (3, 6), (6, 8)]), (4, [(0, 4), (4, 8)]), (8, [(0, 8)]),
                                    (16, [(0, 8)])])
def test_planner_boundaries(c, want):
    plan = chunked.plan_chunks(8, c)
    assert plan == want
    assert plan[0][0] == 0 and plan[-1][1] == 8 and all(a[1] == b[0] for a, b in zip(plan, plan[1:]))    # in order, no gap, no overlap
    assert all(0 < hi - lo <= c for lo, hi in plan) and all(hi - lo == min(c, 8) for lo, hi in plan[:-1])  # only the last may be short


def test_inputs_are_sliced_as_views():
    x = torch.arange(24.0).reshape(8, 3)
    text = {"input_ids": torch.arange(16).reshape(8, 2), "attention_mask": torch.ones(8, 2, dtype=torch.long)}
    xs, ts = chunked.slice_rows(x, 3, 6), chunked.slice_rows(text, 6, 8)
    assert xs.data_ptr() == x[3:].data_ptr() and xs.shape == (3, 3) and chunked.slice_rows(None, 0, 4) is None
    assert sorted(ts) == sorted(text) and ts["input_ids"].data_ptr() == text["input_ids"][6:].data_ptr() and ts["input_ids"].shape == (2, 2)
    assert chunked.batch_rows([None, text, x]) == 8 and chunked.batch_rows([x]) == 8
    with pytest.raises(TypeError):
        chunked.slice_rows("rows", 0, 1)
    with pytest.raises(ValueError):
        chunked.batch_rows([None, None])


# ---- validation -------------------------------------------------------------------------------------------------------------------------------
BAD = [0, -1, -8, True, False, 2.0, 0.5, "4"]


@pytest.mark.parametrize("bad", BAD)
def test_bad_chunk_sizes_raise_value_error(bad):
    from clibd_amd.simclr import SimCLR
    from clibd_amd.train import Trainer

    with pytest.raises(ValueError):
        chunked.validate_chunk_size(bad, "test")
    with pytest.raises(ValueError):
        chunked.plan_chunks(8, bad)
    with pytest.raises(ValueError):          # refused before the model is looked at: nothing here needs a GPU
        Trainer(None, chunk_size=bad)
    with pytest.raises(ValueError):
        SimCLR(chunk_size=bad)


def test_good_chunk_sizes_and_the_fp8_recalibration_combination():
    from clibd_amd.train import Trainer

    assert chunked.validate_chunk_size(None, "test") is None
    assert [chunked.validate_chunk_size(c, "test") for c in (1, 7, 1 << 20)] == [1, 7, 1 << 20]
    with pytest.raises(ValueError, match="fp8_recalibrate_every"):
        Trainer(None, chunk_size=4, fp8_recalibrate_every=10)
    with pytest.raises(ValueError):
        chunked.plan_chunks(0, 4)


def test_documents_and_docstrings_point_at_the_chunked_step():
    from pathlib import Path

    from clibd_amd import optim, simclr, train

    root = Path(__file__).resolve().parents[1]
    design = (root / "DESIGN.md").read_text()
    assert design.index("### 3.18") < design.index("### 3.19") < design.index("## 4. Oracle")
    sec = design[design.index("### 3.19"):design.index("## 4. Oracle")]
    for word in ("GradCache", "replay", "train_arithmetic", "record_stream", "all-gather", "reduce-scatter", "fp8_recalibrate_every", "replay_mismatch",
                 "profiles/chunked_step.log", "bench_chunked_step.py", "Unmeasured"):
        assert word in sec, word
    assert "would be another feature" not in design and "is another feature" not in design[design.index("### 3.18"):]
    for doc in (train.Trainer.__init__.__doc__, simclr.SimCLR.__doc__, optim.__doc__, chunked.__doc__):
        assert "§3.19" in doc and "another feature" not in doc
    assert "chunk_size" in (root / "README.md").read_text()
    assert (root / "tools" / "bench_chunked_step.py").exists() and (root / "profiles" / "chunked_step.log").exists()


# ---- the generator protocol -------------------------------------------------------------------------------------------------------------------
class StubTower:
    """draws its base from the CPU generator inside every forward, as BertTower._forward does in train mode; the base enters the output"""

    def __init__(self, draws):
        self.w = torch.nn.Parameter(torch.tensor([[1.0, 2.0], [0.5, -1.0]]))
        self.draws = draws
        self.on_grads_ready = "hook"            # whatever the trainer installed: must be None for every chunk but the last, and come back

    def __call__(self, x):
        base = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
        self.draws.append((torch.is_grad_enabled(), x.shape[0], base, self.on_grads_ready))
        return (x @ self.w) * (1.0 + (base % 7))


def test_pass_2_sees_the_draws_of_pass_1_and_the_generator_ends_where_pass_1_left_it():
    draws = []
    tw = StubTower(draws)
    x = torch.arange(16.0).reshape(8, 2) / 16.0
    torch.manual_seed(77)
    want = [int(torch.randint(0, 2 ** 31 - 1, (1,)).item()) for _ in range(3)]       # the documented order: one draw per chunk, chunk after chunk
    after_pass_1 = torch.get_rng_state()
    torch.manual_seed(77)
    guard = chunked.ReplayGuard("cpu")
    loss, caches = chunked.two_pass(lambda xc: (tw(xc), None), (x,), 3, lambda leaves: (leaves[0] ** 2).sum(), towers=[tw], guard=guard)
    assert [d[:3] for d in draws] == [(False, 3, want[0]), (False, 3, want[1]), (False, 2, want[2]),      # pass 1: no grad, ragged 3 + 3 + 2
                                      (True, 3, want[0]), (True, 3, want[1]), (True, 2, want[2])]         # pass 2: the same bases, with grad
    assert len(set(want)) == 3
    assert torch.equal(torch.get_rng_state(), after_pass_1)
    assert [d[3] for d in draws[3:]] == [None, None, "hook"] and tw.on_grads_ready == "hook"             # hooks inert until the last chunk
    assert int(guard.mismatch) == 0 and caches[1] is None and caches[0].shape == (8, 2) and not caches[0].requires_grad
    # the accumulated gradient is the full batch's with those bases
    s = torch.cat([torch.full((hi - lo, 1), 1.0 + (b % 7)) for (lo, hi), b in zip(chunked.plan_chunks(8, 3), want)])
    w = tw.w.detach().clone().requires_grad_(True)
    ref = (((x @ w) * s) ** 2).sum()
    ref.backward()
    assert torch.allclose(tw.w.grad, w.grad, rtol=1e-6, atol=0) and torch.allclose(loss, ref.detach(), rtol=1e-6, atol=0)


def test_guard_counts_words_that_pass_2_did_not_reproduce():
    calls = []

    def forward(xc):
        calls.append(xc.shape[0])
        y = xc * w
        if len(calls) == 4:                      # the second chunk of pass 2 comes out different in two words
            y = y + torch.tensor([[0.0, 1.0], [1.0, 0.0], [0.0, 0.0]])
        return (y,)

    w = torch.nn.Parameter(torch.ones(2))
    guard = chunked.ReplayGuard("cpu")
    chunked.two_pass(forward, (torch.ones(6, 2),), 3, lambda leaves: leaves[0].sum(), guard=guard)
    assert calls == [3, 3, 3, 3] and guard.mismatch.dtype == torch.int64 and int(guard.mismatch) == 2
