"""Plain-torch statement of Multi_BTSUNet, the oracle of the HIP model in tests/test_mt_btsunet_*.py.

Written from the architecture (four encoder levels of two conv3x3 -> InstanceNorm -> LeakyReLU(0.01) cells joined by 2 x 2 max-pools, a
bottleneck level plus a one-cell bridge over [e4, bottleneck], three decoder levels fed by nearest 2x up-sampling and the encoder skip, a
classification branch over [e4, bottleneck, cell(bridge)] flattened into Linear(8 * width * 256 -> 256) -> ReLU -> Linear(256 -> logits), 1x1 /
ConvT + 1x1 segmentation heads) with the reference's parameter names, so that a state_dict moves between the two.  It lives here and not
under oracle/ because the GPU tests need it where no reference checkout exists; tests/test_mt_btsunet_cpu.py ties it to the reference's own
numbers (tests/golden/mt_btsunet_step.npz, written by tools/make_btsunet_fixture.py from the reference's classes).

`lowp` ('bf16' | 'f16' | None): under oracle.torch_oracle.lowp_conv3x3 the patched F.conv2d rounds the operands of every 3x3 conv whose
input AND output channel counts are multiples of 8; the product's forward MFMAs need only the INPUT channels in groups of 8 (engine
conv_cell: `use_packed`), so the one cell with 8 -> 4 channels (decoder1's second cell at width 8) is rounded here, by the emulation's own
autograd function, when `lowp` names the mode.  Its output has no 16-bit storage (engine: z16 needs Cout % 8 == 0)."""
from __future__ import annotations

import hashlib
from collections import OrderedDict

import torch
import torch.nn as nn
import torch.nn.functional as F

_LP = {"bf16": torch.bfloat16, "f16": torch.float16}


class _Cell(nn.Module):
    def __init__(self, cin: int, cout: int, owner):
        super().__init__()
        self.Conv = nn.Conv2d(cin, cout, 3, padding=1, bias=False)
        self._owner = [owner]          # (a list: not a sub-module)

    def forward(self, x):
        w = self.Conv.weight
        lowp = self._owner[0].lowp
        H, W = x.shape[-2:]
        if lowp and w.shape[1] % 8 == 0 and w.shape[0] % 8 != 0 and H >= 8 and W >= 8 and W % 4 == 0:
            from oracle.torch_oracle import _LowpConv3x3
            z = _LowpConv3x3.apply(x, w, None, _LP[lowp], None)
        else:
            z = F.conv2d(x, w, None, 1, 1)
        return F.leaky_relu(F.instance_norm(z, eps=1e-5), 0.01)


class _Level(nn.Module):
    def __init__(self, cin: int, cmid: int, cout: int, owner):
        super().__init__()
        self.ConvInNormLRelu1 = _Cell(cin, cmid, owner)
        self.ConvInNormLRelu2 = _Cell(cmid, cout, owner)

    def forward(self, x):
        return self.ConvInNormLRelu2(self.ConvInNormLRelu1(x))


class OracleMultiBTSUNet(nn.Module):
    def __init__(self, sequences: int, regions: int, n_classes: int, width: int, deep_supervision: bool):
        super().__init__()
        self.lowp = None
        self.deep_supervision = deep_supervision
        w = [width, 2 * width, 4 * width, 8 * width]
        logits = 1 if n_classes == 2 else n_classes
        self.encoder1 = _Level(sequences, w[0] // 2, w[0], self)
        self.encoder2 = _Level(w[0], w[1] // 2, w[1], self)
        self.encoder3 = _Level(w[1], w[2] // 2, w[2], self)
        self.encoder4 = _Level(w[2], w[3] // 2, w[3], self)
        self.bottleneck = _Level(w[3], w[3], w[3], self)
        self.bottleneck2 = _Cell(2 * w[3], w[2], self)
        self.decoder3 = _Level(2 * w[2], w[2], w[1], self)
        self.decoder2 = _Level(2 * w[1], w[1], w[0], self)
        self.decoder1 = _Level(2 * w[0], w[0], w[0] // 2, self)
        self.process_bottleneck2 = _Cell(w[2], w[3], self)
        self.process_features_map = _Cell(3 * w[3], w[3], self)
        self.classifier = nn.Sequential(nn.Flatten(), nn.Linear(w[3] * 16 * 16, 256), nn.ReLU(), nn.Linear(256, logits))
        if deep_supervision:
            self.output3 = nn.Sequential(nn.ConvTranspose2d(w[1], w[1], 4, stride=4), nn.Conv2d(w[1], regions, 1))
            self.output2 = nn.Sequential(nn.ConvTranspose2d(w[0], w[0], 2, stride=2), nn.Conv2d(w[0], regions, 1))
        self.output1 = nn.Conv2d(w[0] // 2, regions, 1)
        for m in self.modules():           # the reference's initialisation pass: Conv2d only
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, nonlinearity="leaky_relu")
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)

    def forward(self, x):
        up = lambda t: F.interpolate(t, scale_factor=2, mode="nearest")      # noqa: E731
        e1 = self.encoder1(x)
        e2 = self.encoder2(F.max_pool2d(e1, 2, 2))
        e3 = self.encoder3(F.max_pool2d(e2, 2, 2))
        e4 = self.encoder4(F.max_pool2d(e3, 2, 2))
        b = self.bottleneck(e4)
        b2 = self.bottleneck2(torch.cat([e4, b], 1))
        d3 = self.decoder3(torch.cat([e3, up(b2)], 1))
        d2 = self.decoder2(torch.cat([e2, up(d3)], 1))
        d1 = self.decoder1(torch.cat([e1, up(d2)], 1))
        feat = self.process_features_map(torch.cat([e4, b, self.process_bottleneck2(b2)], 1))
        logits = self.classifier(feat)
        if self.deep_supervision:
            return [logits], [self.output3(d3), self.output2(d2), self.output1(d1)]
        return logits, self.output1(d1)


def state_sha256(state_dict) -> str:
    """sha256 over (name, float32 bytes) of a state_dict in its own order: what tests/golden/mt_btsunet_step.npz records of the reference's
    initial weights."""
    h = hashlib.sha256()
    for k, v in state_dict.items():
        h.update(k.encode())
        h.update(v.detach().cpu().float().contiguous().numpy().tobytes())
    return h.hexdigest()


# the two configurations of the fixture: name -> (width, n_classes, deep_supervision)
CONFIGS = OrderedDict([("w8_c3_ds", (8, 3, True)), ("w16_c2", (16, 2, False))])
ALPHA = 0.35
# the gradients the fixture records; a tensor of more than SAMPLE elements is recorded at SAMPLE fixed flat positions (`sample_index`)
GRAD_TENSORS = ("encoder1.ConvInNormLRelu1.Conv.weight", "bottleneck2.Conv.weight", "process_features_map.Conv.weight", "classifier.3.bias",
                "output1.weight")
SAMPLE = 1024


def sample_index(numel: int, salt: int) -> torch.Tensor:
    """The flat positions of a large tensor that the fixture records: all of them up to SAMPLE elements, else SAMPLE distinct ones drawn once
    from a fixed seed (sorted).  Heads (2 x 128 x 128) are recorded the same way."""
    if numel <= SAMPLE:
        return torch.arange(numel)
    g = torch.Generator().manual_seed(1993 + salt)
    return torch.randperm(numel, generator=g)[:SAMPLE].sort().values
