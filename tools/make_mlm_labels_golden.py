"""Generate tests/golden/mlm_labels_golden.pt: HF transformers' BertForMaskedLM(input_ids, attention_mask, labels), fp32, eval mode, CPU.

    python tools/make_mlm_labels_golden.py        # needs `transformers`; nothing outside this repository is read

Six cases: three shapes (tests/mlm_labels_reference.CASES), each with tie_word_embeddings True and False, B = 4:
  A17   hidden 64, 2 layers, 1 head, intermediate 128, vocabulary 259, 136 positions;  S = 17
  A33   the same model;  S = 33
  D133  hidden 128, 1 layer, 2 heads (64 wide), intermediate 256, vocabulary 259;  S = 133
The inputs are mlm_labels_reference.case_inputs(name): a ragged attention mask (a full row, a row with one live key beyond position 0, a
prefix of half the sequence, a full row with a hole) and labels with many, one, no and many positions per sequence, position 0 and a
masked-out position among them.  Models are built with pad_token_id=None, weights are mlm_reference.synth_state's and are not stored
(a sha256 over them is), and gradients are stored as tests/golden/make_mlm_golden.py stores them: at most 512 hashed entries of each
(mlm_reference.sampled) and every tensor's L2 norm.
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mlm_labels_reference as LR  # noqa: E402
import mlm_reference as MR  # noqa: E402

from transformers import BertConfig, BertForMaskedLM  # noqa: E402


def main():
    out = {}
    for ci, (name, cfg, S) in enumerate(LR.CASES):
        ids, mask, labels = LR.case_inputs(name)
        per_seq = (labels != LR.IGNORE).sum(dim=1).tolist()
        assert per_seq[0] >= 2 and per_seq[1] == 1 and per_seq[2] == 0 and per_seq[3] >= 4, per_seq
        for tied in (True, False):
            seed = 700 + 10 * ci + int(tied)
            hf = BertForMaskedLM(BertConfig(tie_word_embeddings=tied, pad_token_id=None, **cfg)).eval()
            assert hf.bert.embeddings.word_embeddings.padding_idx is None
            sd = MR.synth_state(seed, {k: tuple(v.shape) for k, v in hf.state_dict().items()})
            if tied:
                sd["cls.predictions.decoder.weight"] = sd["bert.embeddings.word_embeddings.weight"]
                sd["cls.predictions.decoder.bias"] = sd["cls.predictions.bias"]
            hf.load_state_dict(sd, strict=True)
            res = hf(input_ids=ids, attention_mask=mask, labels=labels)
            lab = labels.reshape(-1)
            on = lab != LR.IGNORE
            hits = int((res.logits.reshape(-1, cfg["vocab_size"])[on].argmax(-1) == lab[on]).sum())
            ps = dict(hf.named_parameters(remove_duplicate=False))
            uniq = list({id(q): q for q in ps.values()}.values())
            gs = dict(zip(map(id, uniq), torch.autograd.grad(res.loss, uniq, allow_unused=True)))
            grads = {k: (torch.zeros_like(q) if gs[id(q)] is None else gs[id(q)]).detach() for k, q in ps.items()}
            out[(name, tied)] = dict(config=dict(cfg), seed=seed, tied=tied, weights_sha256=MR.state_hash(sd), S=S, input_ids=ids,
                                     attention_mask=mask, labels=labels, n_labelled=int(on.sum()), loss=float(res.loss.detach()), hits=hits,
                                     grads={k: MR.sampled(k, g) for k, g in grads.items()},
                                     grad_norms={k: float(g.double().norm()) for k, g in grads.items()})
            print(f"[make_mlm_labels_golden] {name} tied={tied}: loss {float(res.loss.detach()):.6f}, hits {hits}/{int(on.sum())}, labels per sequence {per_seq}")
    path = os.path.join(ROOT, "tests", "golden", "mlm_labels_golden.pt")
    torch.save(out, path)
    print(f"[make_mlm_labels_golden] {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
