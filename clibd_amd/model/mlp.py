"""`MLPEncoder` and `MLPVersionCLIP`: drop-in for `bioscanclip.model.mlp` (reference model/mlp.py:11-37) on the MI355X HIP engine: the
towers over pre-extracted `image_features` / `dna_features` rows (`input_type: feature`, util/dataset.py:224-266).

The parameter holder is the reference's own `nn.Sequential(Linear, ReLU, Linear, ReLU, Linear)` named `encoder`, so state-dict keys
(`encoder.{0,2,4}.{weight,bias}`) and torch's default initialisation under a seed are the reference's; the arithmetic runs through
`clibd_amd.towers.MLPTower`.
"""
from __future__ import annotations

import torch.nn as nn

from ..towers import MLPTower


class MLPEncoder(nn.Module):
    def __init__(self, input_dim, hidden_dim=512, output_dim=512):
        super().__init__()
        self.encoder = nn.Sequential(
            nn.Linear(input_dim, hidden_dim),
            nn.ReLU(),
            nn.Linear(hidden_dim, hidden_dim),
            nn.ReLU(),
            nn.Linear(hidden_dim, output_dim),
        )
        self._tower = MLPTower([self.encoder[0], self.encoder[2], self.encoder[4]])   # raises NotSupportedYet for widths the kernels do not take

    def tower(self) -> MLPTower:
        return self._tower

    def forward(self, x):
        tw = self.tower()
        tw.training = self.training
        return tw(x)


class MLPVersionCLIP(nn.Module):
    def __init__(self, image_input_dim=512, dna_input_dim=768, hidden_dim=512, output_dim=512):
        super().__init__()
        self.image_feature_encoder = MLPEncoder(input_dim=image_input_dim, hidden_dim=hidden_dim, output_dim=output_dim)
        self.dna_feature_encoder = MLPEncoder(input_dim=dna_input_dim, hidden_dim=hidden_dim, output_dim=output_dim)

    def forward(self, image_feature, dna_feature):
        from .simple_clip import l2_normalize

        return l2_normalize(self.image_feature_encoder(image_feature)), l2_normalize(self.dna_feature_encoder(dna_feature))
