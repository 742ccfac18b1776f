"""A plain-torch restatement of `architecture: UnetPlusPlus` (nets.BasicUnetPlusPlus) for the tests: oracle.torch_oracle.OracleMTUNetPlusPlus(
features=...) with its trunk and its four heads only -- process_level_3 and the classifier are taken out after construction, so the parameter
names, their order and (for a seeded RNG) their initial values are those of the product's model -- run in float64 and float32.

UNPINNED, as MTUNetPlusPlus is: the reference builds this model from MONAI's BasicUNetPlusPlus, MONAI is not installed here, and nothing the
reference holds can pin it.  The blocks are those the reference's own MTUNetPlusPlus.py spells out and oracle/torch_oracle.py restates (TwoConv,
Down, UpCat with a transposed conv, InstanceNorm with affine parameters, LeakyReLU 0.1).  INIT_SHA256 below records the initial weights THIS
restatement draws for seed 1993; it is not a number of the reference's.  No test module: pytest does not collect it."""
import hashlib

import torch

from oracle import torch_oracle as O

FEATURES = (32, 32, 64, 128, 256, 32)          # MONAI 1.3.0 BasicUNetPlusPlus's default `features`
HEADS = ("final_conv_0_1", "final_conv_0_2", "final_conv_0_3", "final_conv_0_4")
# sha256 over the float32 bytes of the state dict, in order, of OracleBasicUnetPlusPlus(1, 1, FEATURES, True) after O.seed_everything(1993):
# the restatement's own draw (a change of the draw order shows here); not the reference's
INIT_SHA256 = "c8b689c7e3e253134e061f0a81b121f29bf7b5d5afc7c3907f6ecc0c21b2dc0e"


class OracleBasicUnetPlusPlus(O.OracleMTUNetPlusPlus):
    def __init__(self, in_channels: int = 1, out_channels: int = 1, features=FEATURES, deep_supervision: bool = False):
        super().__init__(in_channels, out_channels, 3, deep_supervision, features)
        del self.process_level_3, self.classifier          # drawn behind the trunk and the heads: taking them out moves nothing
        self.n_classes = 0

    def forward(self, x):
        """MONAI BasicUNetPlusPlus.forward: always a list -- the four heads under deep supervision, [output_0_4] without."""
        cat = lambda *ts: torch.cat(ts, dim=1)          # noqa: E731
        x00 = self.conv_0_0(x)
        x10 = self.conv_1_0(x00)
        x01 = self.upcat_0_1(x10, x00)
        x20 = self.conv_2_0(x10)
        x11 = self.upcat_1_1(x20, x10)
        x02 = self.upcat_0_2(x11, cat(x00, x01))
        x30 = self.conv_3_0(x20)
        x21 = self.upcat_2_1(x30, x20)
        x12 = self.upcat_1_2(x21, cat(x10, x11))
        x03 = self.upcat_0_3(x12, cat(x00, x01, x02))
        x40 = self.conv_4_0(x30)
        x31 = self.upcat_3_1(x40, x30)
        x22 = self.upcat_2_2(x31, cat(x20, x21))
        x13 = self.upcat_1_3(x22, cat(x10, x11, x12))
        x04 = self.upcat_0_4(x13, cat(x00, x01, x02, x03))
        o4 = self.final_conv_0_4(x04)
        if self.deep_supervision:
            return [self.final_conv_0_1(x01), self.final_conv_0_2(x02), self.final_conv_0_3(x03), o4]
        return [o4]


def sha256_of(state_dict) -> str:
    h = hashlib.sha256()
    for v in state_dict.values():
        h.update(v.detach().cpu().float().contiguous().numpy().tobytes())
    return h.hexdigest()


def seg_loss(outputs, mask, inversely_weighted: bool = True) -> torch.Tensor:
    """criterions.py:27-49 with the Dice criterion of experiment_init.py:210-211: the heads weighted 1 / (j + 1) from the last one backwards."""
    terms = [O.dice_loss_sigmoid_sq(s, mask) / ((j + 1) if inversely_weighted else 1) for j, s in enumerate(reversed(list(outputs)))]
    return torch.sum(torch.stack(terms))


def train_step(model, optimizer, image, mask, inversely_weighted: bool = True):
    """training_segmentation.py:40-57 -> (loss, the list of heads); the optimizer has stepped."""
    optimizer.zero_grad(set_to_none=True)
    outputs = model(image)
    loss = seg_loss(outputs, mask, inversely_weighted)
    if torch.isnan(loss):
        raise SystemExit(1)
    loss.backward()
    optimizer.step()
    return loss.detach(), [o.detach() for o in outputs]
