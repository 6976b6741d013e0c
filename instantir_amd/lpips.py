"""LPIPS v0.1 (net = vgg) on the device: the perceptual distance the reference builds as `lpips.LPIPS(net='vgg')`
(losses/losses.py:81-95), scored on restored images like `metrics.psnr` / `metrics.ssim` (DESIGN.md section 7 "LPIPS").

    from instantir_amd.lpips import LPIPS
    model = LPIPS.from_files("vgg16.pth", "vgg.pth", device="cuda:0")     # torchvision VGG-16 + lpips' lin layers
    model = LPIPS.from_files("lpips_vgg_full.pth", device="cuda:0")       # or one whole `lpips.LPIPS` state dict
    model(restored, gt)                       # fp64 (N,) on the device; layers=True: (N, 5); spatial=True: + the five maps

The contract: both images go to [-1, 1] and through the scaling layer (`ops.lpips_prep`), then through the thirteen 3x3 convs of
VGG-16 `features` (`ops.conv2d` with a bias and ACT_NONE, the `a` and the `b` image of a pair stacked as one batch of two so
that each weight is read once), ReLU after each (`ops.relu_`, or inside `ops.lpips_tap`), 2x2 max pools between the five
slices.  The ReLU outputs after convs 2, 7, 14, 21 and 28 are the taps: each is unit-normalised over channels per pixel, the
squared difference is weighted by the non-negative 1x1 `lin` layer and averaged over the tap's pixels, and LPIPS is the sum of
the five (`ops.lpips_tap`, which also writes the pooled activations the next slice reads).  Pairs are processed one at a time
from one activation arena, so memory does not grow with the batch.  There is no host path.

No real LPIPS weights exist offline: the two file formats are read as the packages write them to the best of public
knowledge, and `LPIPS.synthetic` / `synthetic_state_dict` draw seeded stand-ins the CPU restatement of the tests rebuilds.
"""
from __future__ import annotations

import torch

from . import ops
from .vgg import VGG_WIDTHS, PairModel, get_tensor, load_state_dicts, pair_view, read_convs, read_triples, slice_widths, synthetic_convs


def synthetic_state_dict(seed, widths=VGG_WIDTHS):
    """A whole-`lpips.LPIPS` state dict (format (b) of `parse_state_dict`) of seeded fp32 CPU tensors: He-initialised convs
    (N(0, 2 / fan_in)), biases 0.02 N(0, 1), lin weights uniform in [0, 1) -- all drawn in this order from one
    torch.Generator, the way tests/golden/seeded.py fills its modules."""
    g = torch.Generator()
    g.manual_seed(int(seed))
    sd, widths = synthetic_convs(g, widths, lambda k, i: f"net.slice{k}.{i}", "LPIPS")
    for l, c in enumerate(widths):
        sd[f"lin{l}.model.1.weight"] = torch.rand(1, c, 1, 1, generator=g)
    return sd


def parse_state_dict(sd, lin_sd=None):
    """-> (convs, lins, shift, scale): thirteen (weight (Cout, Cin, 3, 3), bias (Cout,)) pairs in execution order, five lin
    vectors (C,), and the scaling layer, all fp32 on the CPU.  Two formats, told apart by their keys:
      (a) a torchvision VGG-16 state dict (`features.{i}.weight` / `.bias`) plus `lin_sd`, lpips' `vgg.pth`
          (`lin{l}.model.1.weight`, shaped (1, C, 1, 1));
      (b) a whole `lpips.LPIPS` state dict: `net.slice{k}.{i}.weight` / `.bias` with the same i, `lin{l}.model.1.weight`
          (duplicates under `lins.{l}.` are ignored), optional `scaling_layer.shift` / `scaling_layer.scale`.
    Widths come from the tensors.  A missing key, a kernel that is not 3x3, a width that is not a multiple of 8 and a channel
    count that does not follow from the layer before raise ValueError naming the key."""
    whole = any(k.startswith("net.slice") for k in sd)
    lin_src = sd if whole else lin_sd
    if lin_src is None:
        raise ValueError("LPIPS weights: a torchvision VGG-16 state dict needs the lin layers too (lin_path: lpips' vgg.pth, "
                         "keys lin{l}.model.1.weight)")
    who = "LPIPS weights"
    convs, lins = read_convs(sd, "net.slice{k}.{i}" if whole else None, who), []
    for l, c in enumerate(slice_widths(convs)):
        key = f"lin{l}.model.1.weight"
        lin = get_tensor(lin_src, key, who)
        if lin.numel() != c or tuple(lin.shape) not in ((1, c, 1, 1), (c,)):
            raise ValueError(f"LPIPS weights: {key} must be shaped (1, {c}, 1, 1), got {tuple(lin.shape)}")
        lins.append(lin.reshape(c).contiguous())
    shift, scale = read_triples(sd if whole else {}, ("scaling_layer.shift", "scaling_layer.scale"), (ops.LPIPS_SHIFT, ops.LPIPS_SCALE), who)
    return convs, lins, shift, scale


def load_weights(path, lin_path=None):
    """`parse_state_dict` of one or two files, each read with safetensors or `torch.load(..., weights_only=True)` on the CPU."""
    return load_state_dicts(parse_state_dict, path, lin_path)


class LPIPS(PairModel):
    """`from_state_dict(sd, lin_sd)`, `from_files(vgg_or_lpips_path, lin_path)` and `synthetic(seed, widths)` build one."""
    NAME, MODULE, WHY = "LPIPS", "instantir_amd.lpips", "four 2x2 pools must leave the fifth tap a pixel"
    parse_state_dict, synthetic_state_dict = staticmethod(parse_state_dict), staticmethod(synthetic_state_dict)

    def __init__(self, convs, lins, shift=ops.LPIPS_SHIFT, scale=ops.LPIPS_SCALE, device=None, dtype=torch.float16):
        super().__init__(convs, device, dtype)
        self.lin = []
        for lin, cp in zip(lins, self.padded):
            lp = torch.zeros(cp, dtype=torch.float32)
            lp[:lin.numel()] = lin
            self.lin.append(lp.to(self.device))
        self.shift, self.scale = tuple(shift), tuple(scale)
        self.affine = ops.lpips_affine(self.device, shift, scale)

    def tap_sizes(self, H, W):
        """(H_l, W_l) of the five taps: floor halving after each of the first four."""
        return [(H >> l, W >> l) for l in range(5)]

    def _pair(self, a, b, H, W, out, maps):
        """One pair through the network: a, b sources of one image each; out fp64 (5, 1) views; maps: five (1, H_l, W_l) or None."""
        sizes = self.tap_sizes(H, W)

        def tap(l, x, H, W, other):
            pooled = pair_view(other, *sizes[l + 1], x.shape[1]) if l < 4 else None
            ops.lpips_tap(x, 1, H, W, self.lin[l], pooled=pooled, dmap=None if maps is None else maps[l], out=out[l])
            return pooled
        self._trunk(a, b, sizes, tap)

    def __call__(self, a, b, layers=False, spatial=False):
        """LPIPS of `a` against `b`, each what `metrics.psnr` accepts (a PIL image or a list of them, a numpy array, a tensor; 3
        channels, [0, 1] scale or 8-bit).  Returns fp64 (N,) on the device, (N, 5) with `layers` (the five taps' terms, whose sum
        over the row is the score); with `spatial` a pair (that, [five fp32 (N, H_l, W_l) maps of the per-pixel terms])."""
        ta, tb, (N, H, W) = self._upload(a, b)
        res = torch.empty(5, N, dtype=torch.float64, device=self.device)
        maps = [torch.empty(N, h, w, dtype=torch.float32, device=self.device) for h, w in self.tap_sizes(H, W)] if spatial else None
        for n in range(N):
            self._pair(ta[n:n + 1], tb[n:n + 1], H, W, [res[l, n:n + 1] for l in range(5)],
                       None if maps is None else [m[n:n + 1] for m in maps])
        self._check_finite(res, "tap")
        per_layer = res.t().contiguous()
        score = per_layer if layers else per_layer.sum(dim=1)
        return (score, maps) if spatial else score
