"""Attention rollout of the ViT and BarcodeBERT towers on the device: the arithmetic behind the reference's
scripts/result/representation_visualization/image_representation_visualization.py and dna_representation_visualization.py (`rollout`, after
jacobgil/vit-explain), i.e. "what does the encoder look at, before and after alignment".

The reference hooks every layer's attention dropout, copies [1, heads, S, S] probabilities per layer to the host, fuses the heads, drops
the lowest `discard_ratio` of each fused map and chains the maps.  The towers here have no such module and their attention kernels never
hold the probabilities in memory, so the arithmetic is rebuilt from what the tower's forward records per layer, the packed `qkv`:

  * clibd_attn_fused_maps   per head softmax(q k^T / 8) recomputed, the heads fused in registers (mean / max / min): [S, S] per layer
  * clibd_rollout_discard   the k = int(S * S * discard_ratio) smallest entries of a map zeroed, exactly; flat index 0 counts among the k
                            but keeps its value (the reference's `indices[indices != 0]`)
  * clibd_rollout_chain     a = (F + I) / 2, a[i, j] /= sum_k a[j, k] (the reference divides COLUMN j by the sum of ROW j: its divisor has
                            shape [1, S] and broadcasts over the last axis), result = a @ result; only row 0 is read, so the chain is a
                            vector-matrix walk from the last selected layer to the first; mask = row[1:] / max(row[1:])

(include/clibd_hip_rollout.h).  Device forms: `fused_attention_maps`, `rollout_from_maps`, `attention_rollout` (tensors in, tensors out,
no host synchronisation).  Reference-named classes: `VITAttentionRollout`, `BarcodeBERTAttentionRollout` (numpy masks, as the scripts'
get_and_save_vit_explaination and get_attention_mask expect).

Layer windows with layer_idx=None, as in the two scripts: the ViT uses attentions[1:-6] (layers 1..5 of 12), BarcodeBERT attentions[1:];
layer_idx = i uses layer i alone.

Stated divergences from the reference:
  * a batch is B independent B = 1 calls (for B > 1 the reference applies the union of every sample's indices to sample 0 and its division
    fails to broadcast);
  * an empty layer window (fewer than 8 layers under [1:-6], a layer_idx outside the tower) raises ValueError; the reference returns 0/0;
  * an unknown head fusion raises ValueError (the reference raises a string);
  * ties at the k-th smallest value, which torch.topk leaves unspecified: entries equal to it are zeroed in ascending flat index;
  * the text tower and key masks are not covered: the reference has no such rollout;
  * under the fp8 forward on every site with trainable base weights the tower's recording forward raises NotSupportedYet;
  * a tower whose heads are not 64 wide (the newer BarcodeBERT checkpoints: 128 / 192) raises NotSupportedYet: the map kernel reads 64-wide heads;
  * no heat-map overlay and no drawing (cv2 and matplotlib are out of scope, as for the other result scripts).
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch

from . import ops
from .engine import NotSupportedYet

FUSIONS = {"mean": ops.FUSE_MEAN, "max": ops.FUSE_MAX, "min": ops.FUSE_MIN}
VIT_WINDOW = slice(1, -6)     # image_representation_visualization.py: attentions[1:-6]
DNA_WINDOW = slice(1, None)   # dna_representation_visualization.py: attentions[1:]
MAX_IMAGES_PER_FORWARD = 64   # the recording forward keeps every layer's activations: larger batches go in chunks


def _fusion_code(head_fusion: str) -> int:
    if head_fusion not in FUSIONS:
        raise ValueError(f"Attention head fusion type Not supported: {head_fusion!r} (have {sorted(FUSIONS)})")
    return FUSIONS[head_fusion]


def select_layers(n_layers: int, layer_idx: Optional[int] = None, window: slice = VIT_WINDOW) -> List[int]:
    """the layers the reference's rollout walks, in its order: attentions[window] or attentions[layer_idx:layer_idx + 1]; an empty
    selection raises ValueError"""
    layers = list(range(int(n_layers)))
    sel = layers[window] if layer_idx is None else layers[int(layer_idx):int(layer_idx) + 1]
    if not sel:
        raise ValueError(f"attention rollout: no layer selected (layers {n_layers}, layer_idx {layer_idx}, window {window})")
    return sel


def discard_count(S: int, discard_ratio: float) -> int:
    """the reference's int(flat.size(-1) * discard_ratio), in Python float arithmetic"""
    k = int(S * S * discard_ratio)
    if not 0 <= k <= S * S:
        raise ValueError("attention rollout: discard_ratio must lie in [0, 1]")
    return k


def fused_attention_maps(qkv: torch.Tensor, B: int, S: int, heads: int, fusion: str) -> torch.Tensor:
    """fp32 [B, S, S] (a view of the padded [B, S, ld] buffer): the heads' softmax(q k^T / 8) of one layer fused by `fusion`; qkv is the
    layer's packed bf16 [B * S, 3 * 64 * heads] (what TransformerStack.forward(save=True) records as rec["qkv"])."""
    return ops.attn_fused_maps(qkv, B, S, heads, _fusion_code(fusion))[:, :, :S]


def rollout_from_maps(maps: torch.Tensor, discard_ratio: float) -> torch.Tensor:
    """fp32 [B, S - 1]: discard + chain of fused maps fp32 [L, B, S, S] given in the order of application.  `maps` is not changed."""
    if maps.dim() != 4 or maps.shape[2] != maps.shape[3]:
        raise ValueError("rollout_from_maps: maps must be [L, B, S, S]")
    L, B, S, _ = maps.shape
    k = discard_count(S, discard_ratio)
    buf = torch.zeros((L, B, S, ops.rollout_ld(S)), dtype=torch.float32, device=maps.device)
    buf[..., :S].copy_(maps)
    ops.rollout_discard_(buf, S, k)
    return ops.rollout_chain(buf, S)


def _encoder_kind(encoder) -> str:
    from .model.dna_encoder import CLIBDDNAEncoder
    from .model.image_encoder import CLIBDImageEncoder

    if isinstance(encoder, CLIBDImageEncoder):
        return "vit"
    if isinstance(encoder, CLIBDDNAEncoder):
        return "dna"
    raise TypeError("attention rollout: the encoder must be a CLIBDImageEncoder or a CLIBDDNAEncoder")


def _tower_inputs(kind: str, x: torch.Tensor) -> tuple:
    """the inputs tuple of the tower's _forward: an image batch, or (token ids, no token types, no key mask)"""
    return (x,) if kind == "vit" else (x, None, None)


def attention_rollout(encoder, inputs: torch.Tensor, head_fusion: str = "min", discard_ratio: float = 0.9, layer_idx: Optional[int] = None,
                      window: Optional[slice] = None) -> torch.Tensor:
    """fp32 [B, S - 1] on the device: the rollout mask of every input of the batch.  encoder: CLIBDImageEncoder (inputs [B, 3, 224, 224]) or
    CLIBDDNAEncoder (token ids [B, S]); window: the layers walked when layer_idx is None (default: the encoder's reference window)."""
    fusion = _fusion_code(head_fusion)
    kind = _encoder_kind(encoder)
    default_window = VIT_WINDOW if kind == "vit" else DNA_WINDOW
    tower = encoder.tower()
    stack = tower.stack
    if getattr(stack, "dh", 64) != 64:   # clibd_attn_fused_maps reads q and k at 64-column strides: it would misread a wide tower's qkv
        raise NotSupportedYet(f"attention rollout is built for head_dim 64 (this tower: {stack.dh})")
    layers = select_layers(len(stack.layers), layer_idx, default_window if window is None else window)
    dev = next(encoder.parameters()).device
    x = inputs.to(dev)
    out = []
    was_training = tower.training
    tower.training = False
    try:
        with torch.no_grad():
            for b0 in range(0, x.shape[0], MAX_IMAGES_PER_FORWARD):
                tin = _tower_inputs(kind, x[b0:b0 + MAX_IMAGES_PER_FORWARD])
                _, state = tower._forward(tin, True)
                qkvs = [state["saved"][i]["qkv"] for i in layers]
                del state   # everything else the recording forward kept
                B = tin[0].shape[0]
                S = qkvs[0].shape[0] // B
                maps = torch.empty((len(layers), B, S, ops.rollout_ld(S)), dtype=torch.float32, device=dev)
                for l, qkv in enumerate(qkvs):
                    ops.attn_fused_maps(qkv, B, S, stack.heads, fusion, out=maps[l])
                del qkvs
                ops.rollout_discard_(maps, S, discard_count(S, discard_ratio))
                out.append(ops.rollout_chain(maps, S))
    finally:
        tower.training = was_training
    return out[0] if len(out) == 1 else torch.cat(out)


class _AttentionRollout:
    """the two reference classes: constructor and call signatures of the scripts; `attention_layer_name` is accepted and ignored (there is
    no module to hook)"""

    window = VIT_WINDOW

    def __init__(self, model, attention_layer_name=None, head_fusion="min", discard_ratio=0.9):
        _encoder_kind(model)   # the encoder type, checked once
        _fusion_code(head_fusion)
        self.model = model
        self.head_fusion = head_fusion
        self.discard_ratio = discard_ratio
        self.hooks: Sequence = []

    def _shape(self, mask: np.ndarray) -> np.ndarray:
        return mask

    def __call__(self, input_tensor, layer_idx=None) -> np.ndarray:
        mask = attention_rollout(self.model, input_tensor, self.head_fusion, self.discard_ratio, layer_idx, self.window)
        mask = self._shape(mask.cpu().numpy())
        return mask[0] if mask.shape[0] == 1 else mask

    def remove_hooks(self):
        """nothing is hooked: kept so that the scripts' clean-up runs unchanged"""
        self.hooks = []


class VITAttentionRollout(_AttentionRollout):
    """image_representation_visualization.VITAttentionRollout: a [w, w] mask (w = int((S - 1) ** 0.5), 14 for ViT-B/16) for one image,
    [B, w, w] for a batch"""

    window = VIT_WINDOW

    def __init__(self, model, attention_layer_name="attn_drop", head_fusion="min", discard_ratio=0.9):
        super().__init__(model, attention_layer_name, head_fusion, discard_ratio)

    def _shape(self, mask):
        w = int(mask.shape[-1] ** 0.5)
        return mask.reshape(mask.shape[0], w, w)


class BarcodeBERTAttentionRollout(_AttentionRollout):
    """dna_representation_visualization.BarcodeBERTAttentionRollout: a flat [S - 1] mask for one sequence, [B, S - 1] for a batch"""

    window = DNA_WINDOW

    def __init__(self, model, attention_layer_name="attention.self.dropout", head_fusion="min", discard_ratio=0.9):
        super().__init__(model, attention_layer_name, head_fusion, discard_ratio)
