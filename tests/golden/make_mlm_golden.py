"""Generate tests/golden/mlm_golden.pt: the masked-LM objective of HF transformers' BertForMaskedLM(input_ids, labels), fp32, eval mode, CPU.

    python tests/golden/make_mlm_golden.py        # needs `transformers`; the reference tree is not involved

Six cases: three shapes, each with tie_word_embeddings True and False.
  A17   hidden 64, 2 layers, 1 head, intermediate 128, vocabulary 259 (k = 4), 136 positions;  B = 3, S = 17
  A133  the same model;  B = 3, S = 133
  C33   hidden 256, 1 layer, 2 heads (128 wide), intermediate 256, vocabulary 1027 (k = 5), 64 positions;  B = 2, S = 33
Labels are -100 except at the rows of tests/mlm_reference.py's sampler (ratio 0.5); in every case one sequence has fewer real k-mers than
masked positions, so some chosen positions hold <UNK> and their targets are -100.
The models are built with pad_token_id=None.  BertConfig's default pad_token_id = 0 is the k-mer vocabulary's <MASK> and makes row 0 of the
word table an nn.Embedding padding row, whose lookup gradient torch drops: the mask token's embedding would never train through the lookup.
The project's embedding backward has no padding row (clibd_amd.mlm says so), and the golden pins that.

The six models hold 1.4 M parameters and as many gradient entries, and a committed file stays far below 1 MiB.  So
  - the weights are not stored: they are a pure integer-arithmetic function of (seed, key, element index) (mlm_reference.synth_state), and
    the file keeps a sha256 over them, which a loader checks after regenerating them;
  - of a gradient with more than 512 entries the file keeps 512 entries at hashed positions (mlm_reference.sample_index) and the L2 norm of the whole
    tensor; smaller gradients are kept whole.
Stored per case: config, seed, weights' hash, ids, masked ids, rows, targets, n_valid, loss, hits (masked-token accuracy = hits / n_valid),
gradient samples and norms under the HF state-dict keys.
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import mlm_reference as MR  # noqa: E402

from transformers import BertConfig, BertForMaskedLM  # noqa: E402

A = dict(vocab_size=259, hidden_size=64, num_hidden_layers=2, num_attention_heads=1, intermediate_size=128, max_position_embeddings=136)
C = dict(vocab_size=1027, hidden_size=256, num_hidden_layers=1, num_attention_heads=2, intermediate_size=256, max_position_embeddings=64)
CASES = [("A17", A, 3, 17, 5), ("A133", A, 3, 133, 40), ("C33", C, 2, 33, 10)]   # name, config, B, S, real k-mers of sequence 1


def golden_state(seed, hf, tied):
    sd = MR.synth_state(seed, {k: tuple(v.shape) for k, v in hf.state_dict().items()})
    if tied:
        sd["cls.predictions.decoder.weight"] = sd["bert.embeddings.word_embeddings.weight"]
        sd["cls.predictions.decoder.bias"] = sd["cls.predictions.bias"]
    return sd


def main():
    out = {}
    for ci, (name, cfg, B, S, real) in enumerate(CASES):
        gen = torch.Generator().manual_seed(77 + ci)
        V = cfg["vocab_size"]
        ids = torch.cat([torch.zeros(B, 1, dtype=torch.long), torch.randint(3, V, (B, S - 1), generator=gen)], dim=1)
        ids[1, 1 + real:] = 2                                  # the padding k-mers of a short barcode
        n_mask = MR.n_mask_for(S, 0.5)
        masked, rows, targets, n_valid = MR.sample(ids, 1234 + ci, n_mask)
        assert (targets == MR.IGNORE).sum() == n_mask - real and int(n_valid) == B * n_mask - (n_mask - real)
        labels = torch.full((B * S,), MR.IGNORE, dtype=torch.long)
        labels[rows.long()] = targets
        for tied in (True, False):
            seed = 500 + 10 * ci + int(tied)
            hf = BertForMaskedLM(BertConfig(tie_word_embeddings=tied, pad_token_id=None, **cfg)).eval()
            assert hf.bert.embeddings.word_embeddings.padding_idx is None
            sd = golden_state(seed, hf, tied)
            hf.load_state_dict(sd, strict=True)
            p = hf.cls.predictions
            assert (p.decoder.weight is hf.bert.embeddings.word_embeddings.weight) == tied and (p.decoder.bias is p.bias) == tied
            res = hf(input_ids=masked, labels=labels.view(B, S))
            hits = int((res.logits.view(B * S, V)[rows.long()].argmax(-1) == targets).sum())
            ps = dict(hf.named_parameters(remove_duplicate=False))
            uniq = list({id(q): q for q in ps.values()}.values())
            gs = dict(zip(map(id, uniq), torch.autograd.grad(res.loss, uniq, allow_unused=True)))
            grads = {k: (torch.zeros_like(q) if gs[id(q)] is None else gs[id(q)]).detach() for k, q in ps.items()}
            out[(name, tied)] = dict(config=dict(cfg), seed=seed, tied=tied, weights_sha256=MR.state_hash(sd), B=B, S=S, n_mask=n_mask, ids=ids,
                                     masked=masked, rows=rows, targets=targets, n_valid=n_valid, loss=float(res.loss.detach()), hits=hits,
                                     grads={k: MR.sampled(k, g) for k, g in grads.items()},
                                     grad_norms={k: float(g.double().norm()) for k, g in grads.items()})
            print(f"[make_mlm_golden] {name} tied={tied}: loss {float(res.loss.detach()):.6f}, hits {hits}/{int(n_valid)}, {len(grads)} gradients")
    path = os.path.join(HERE, "mlm_golden.pt")
    torch.save(out, path)
    print(f"[make_mlm_golden] {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
