"""Generate the wide-head DNA-tower goldens under tests/golden/ by IMPORTING THE REFERENCE (authoring container only).

    python tests/golden/make_wide_head_golden.py      # needs the reference checkout make_golden.py names; writes wide_head_{128,192}_golden.pt

The newer BarcodeBERT checkpoints (k = 4, 6 heads x 6 layers and 4 heads x 4 layers at hidden 768) have 128- and 192-wide heads.  These two
fixtures are the reference's own CLIBDDNAEncoder over HF transformers' BertForMaskedLM, as dna_tiny_golden.pt is (make_golden.py, G2), with
one head of that width: fp32, eval mode, LoRA B matrices non-zero.
  wide_head_128_golden.pt   hidden 128, 1 head, 2 layers, intermediate 256
  wide_head_192_golden.pt   hidden 192, 1 head, 1 layer,  intermediate 384
Both: vocabulary 258 (4^4 4-mers + two specials), 133 tokens, batch 3, 160 positions, 128 output classes.
Every weight is drawn and then rounded to a bf16-representable value BEFORE the reference runs, and the state dict is stored as bfloat16
(exact, half the bytes: each file stays below 1 MiB); a loader widens it with .float() and holds the very weights the reference computed with.
Only DATA (inputs, weights, expected outputs / gradients) is written; no reference source is copied.
"""
import os

import torch

from make_golden import HERE, grads_of, import_reference, randomize_  # noqa: E402  (installs sys.path for the repository root as well)

from transformers import BertConfig, BertForMaskedLM  # noqa: E402

VOCAB, S, B, MAX_POS, CLASSES = 258, 133, 3, 160, 128
SHAPES = {128: dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=1, intermediate_size=256),
          192: dict(hidden_size=192, num_hidden_layers=1, num_attention_heads=1, intermediate_size=384)}


def main():
    ref = import_reference()
    for dh, cfg in SHAPES.items():
        gen = torch.Generator().manual_seed(1000 + dh)
        hf = BertForMaskedLM(BertConfig(vocab_size=VOCAB, max_position_embeddings=MAX_POS, output_hidden_states=True, **cfg))
        enc = ref["dna_encoder"].CLIBDDNAEncoder(model=hf, r=4, num_classes=CLASSES)
        randomize_(enc, gen)
        with torch.no_grad():
            for p in enc.parameters():
                p.copy_(p.bfloat16().float())
        enc.eval()
        ids = torch.cat([torch.zeros(B, 1, dtype=torch.long), torch.randint(2, VOCAB, (B, S - 1), generator=gen)], dim=1)
        y = enc(ids)
        w = torch.randn(y.shape, generator=gen)
        sd = {}
        for k, v in enc.state_dict().items():
            v = v.detach().clone()
            if v.is_floating_point():
                assert torch.equal(v.bfloat16().float(), v), k
                v = v.bfloat16()
            sd[k] = v
        out = {"config": dict(cfg), "vocab": VOCAB, "max_pos": MAX_POS, "state_dict": sd, "ids": ids, "out": y.detach().clone(), "cot": w,
               "grads": grads_of(enc, (y * w).sum())}
        path = os.path.join(HERE, f"wide_head_{dh}_golden.pt")
        torch.save(out, path)
        print(f"[make_wide_head_golden] head_dim {dh}: out {tuple(y.shape)} sum {float(y.detach().sum()):.6f}, trainable {len(out['grads'])}, "
              f"{os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
