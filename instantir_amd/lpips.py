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
from .engine import Arena
from .images import dims, host_source, scoring_device
from .packing import conv_weight_nhwc

CONVS = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)            # torchvision indices of VGG-16 `features`' convs
SLICES = ((0, 2), (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28))  # a 2x2 max pool between slices; each slice's last ReLU is a tap
VGG_WIDTHS = (64, 128, 256, 512, 512)
MIN_SIDE = 16                                                          # four pools: the fifth tap keeps one pixel
DTYPES = {torch.float16: "fp16", torch.bfloat16: "bf16"}


def _pad64(c):
    return (c + 63) // 64 * 64


def get_tensor(src, key, who):
    """`src[key]` as fp32 on the CPU; a missing key raises ValueError naming it (`who`: "LPIPS weights", "DISTS weights")."""
    if key not in src:
        raise ValueError(f"{who}: missing key {key}")
    return src[key].detach().to("cpu", torch.float32)


def get_conv(sd, name, cin, who):
    """(weight (Cout, cin, 3, 3), bias (Cout,)) of the VGG conv stored under `name`, checked: a kernel that is not 3x3, a width
    that is not a multiple of 8 and a channel count that does not follow from the layer before raise ValueError naming the key."""
    w, b = get_tensor(sd, name + ".weight", who), get_tensor(sd, name + ".bias", who)
    if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3):
        raise ValueError(f"{who}: {name}.weight must be a (Cout, Cin, 3, 3) kernel, got {tuple(w.shape)}")
    if w.shape[0] % 8:
        raise ValueError(f"{who}: {name}.weight has {w.shape[0]} output channels, not a multiple of 8")
    if w.shape[1] != cin:
        raise ValueError(f"{who}: {name}.weight reads {w.shape[1]} channels but the layer before it writes {cin}")
    if tuple(b.shape) != (w.shape[0],):
        raise ValueError(f"{who}: {name}.bias must hold {w.shape[0]} values, got {tuple(b.shape)}")
    return w, b


def synthetic_convs(g, widths, name_of, who):
    """The thirteen seeded convs of a stand-in VGG-16 as state-dict entries `name_of(k, i)`: He-initialised weights
    (N(0, 2 / fan_in)) and biases 0.02 N(0, 1), drawn in execution order from the generator `g`."""
    widths = tuple(int(w) for w in widths)
    if len(widths) != 5 or any(w <= 0 or w % 8 for w in widths):
        raise ValueError(f"{who}.synthetic: widths must be five positive multiples of 8, got {widths}")
    sd, cin = {}, 3
    for k, (idx, cout) in enumerate(zip(SLICES, widths), 1):
        for i in idx:
            sd[name_of(k, i) + ".weight"] = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
            sd[name_of(k, i) + ".bias"] = torch.randn(cout, generator=g) * 0.02
            cin = cout
    return sd, widths


def pack_convs(convs, device, dtype):
    """The convs as `ops.conv2d` reads them, on `device`: NHWC weights and biases in `dtype`, every channel count padded to whole
    64-channel K tiles; zero weights and biases keep the padding channels at exactly 0."""
    packed, cin = [], ops.LPIPS_CPAD
    for w, b in convs:
        cout = _pad64(w.shape[0])
        wp = torch.zeros(cout, 3, 3, cin, dtype=dtype)
        wp[:w.shape[0]] = conv_weight_nhwc(w.to(dtype), cin)
        bp = torch.zeros(cout, dtype=dtype)
        bp[:w.shape[0]] = b.to(dtype)
        packed.append((wp.to(device), bp.to(device)))
        cin = cout
    return packed


def pair_buffers(arena, half):
    """The two activation buffers of `half` elements a pair ping-pongs between, from `arena` (grown when it is too small)."""
    need = 2 * ((half + 127) // 128 * 128)
    if arena.buf is None or arena.buf.numel() < need:
        arena.reserve(need)
    arena.reset()
    return arena.alloc(1, half)[0], arena.alloc(1, half)[0]


def check_pair_geometry(who, H, W, nbytes, why):
    """Raised before any launch: a side below MIN_SIDE (`why`); a largest activation of a pair (`nbytes`) of 2 GiB or more, the
    limit of the conv's plain stores."""
    if min(H, W) < MIN_SIDE:
        raise ValueError(f"{who}: the smallest side is {MIN_SIDE} ({why}), got {H}x{W}")
    if nbytes >= 1 << 31:
        raise ValueError(f"{who} of a {H}x{W} pair: its largest activation ({nbytes} bytes) reaches 2 GiB, beyond what the conv "
                         "launches have been verified for; score crops or a smaller size")


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
    get = lambda src, key: get_tensor(src, key, who)
    convs, lins, cin = [], [], 3
    for k, idx in enumerate(SLICES, 1):
        for i in idx:
            convs.append(get_conv(sd, f"net.slice{k}.{i}" if whole else f"features.{i}", cin, who))
            cin = convs[-1][0].shape[0]
        key = f"lin{k - 1}.model.1.weight"
        lin = get(lin_src, key)
        if lin.numel() != cin or tuple(lin.shape) not in ((1, cin, 1, 1), (cin,)):
            raise ValueError(f"LPIPS weights: {key} must be shaped (1, {cin}, 1, 1), got {tuple(lin.shape)}")
        lins.append(lin.reshape(cin).contiguous())
    shift, scale = ops.LPIPS_SHIFT, ops.LPIPS_SCALE
    if whole and "scaling_layer.shift" in sd:
        for key in ("scaling_layer.shift", "scaling_layer.scale"):
            if get(sd, key).numel() != 3:
                raise ValueError(f"LPIPS weights: {key} must hold 3 values, got {tuple(sd[key].shape)}")
        shift = tuple(get(sd, "scaling_layer.shift").double().reshape(3).tolist())
        scale = tuple(get(sd, "scaling_layer.scale").double().reshape(3).tolist())
    return convs, lins, shift, scale


def load_weights(path, lin_path=None):
    """`parse_state_dict` of one or two files, each read with safetensors or `torch.load(..., weights_only=True)` on the CPU."""
    from .loaders import _load_file
    return parse_state_dict(_load_file(path), None if lin_path is None else _load_file(lin_path))


class LPIPS:
    def __init__(self, convs, lins, shift=ops.LPIPS_SHIFT, scale=ops.LPIPS_SCALE, device=None, dtype=torch.float16):
        if dtype not in DTYPES:
            raise ValueError("LPIPS: dtype must be torch.float16 (default) or torch.bfloat16")
        self.device, self.dtype, self.dtype_name = scoring_device(device, "instantir_amd.lpips"), dtype, DTYPES[dtype]
        self.widths = tuple(convs[j][0].shape[0] for j in (1, 3, 6, 9, 12))
        self.padded = tuple(_pad64(c) for c in self.widths)          # the conv reads whole 64-channel K tiles (pack_convs)
        self.w = pack_convs(convs, self.device, dtype)
        self.lin = []
        for lin, cp in zip(lins, self.padded):
            lp = torch.zeros(cp, dtype=torch.float32)
            lp[:lin.numel()] = lin
            self.lin.append(lp.to(self.device))
        self.shift, self.scale = tuple(shift), tuple(scale)
        self.affine = ops.lpips_affine(self.device, shift, scale)
        self.arena = Arena(self.device, dtype)

    @classmethod
    def from_state_dict(cls, sd, lin_sd=None, device=None, dtype=torch.float16):
        return cls(*parse_state_dict(sd, lin_sd), device=device, dtype=dtype)

    @classmethod
    def from_files(cls, vgg_or_lpips_path, lin_path=None, device=None, dtype=torch.float16):
        return cls(*load_weights(vgg_or_lpips_path, lin_path), device=device, dtype=dtype)

    @classmethod
    def synthetic(cls, seed, widths=VGG_WIDTHS, device=None, dtype=torch.float16):
        return cls.from_state_dict(synthetic_state_dict(seed, widths), device=device, dtype=dtype)

    # ---- geometry -----------------------------------------------------------------------------------
    def tap_sizes(self, H, W):
        """(H_l, W_l) of the five taps: floor halving after each of the first four."""
        return [(H >> l, W >> l) for l in range(5)]

    def _largest_activation_bytes(self, H, W):
        return 2 * H * W * max(ops.LPIPS_CPAD, self.padded[0]) * 2

    def _check_geometry(self, H, W):
        """Raised before any launch: a side below 16 leaves the fifth tap without a pixel; the largest activation of a pair (both
        images at full resolution in the first slice's channels) must stay below 2 GiB, the limit of the conv's plain stores."""
        check_pair_geometry("LPIPS", H, W, self._largest_activation_bytes(H, W), "four 2x2 pools must leave the fifth tap a pixel")

    # ---- the network --------------------------------------------------------------------------------
    def _pair(self, a, b, H, W, out, maps):
        """One pair through the network: a, b sources of one image each; out fp64 (5, 1) views; maps: five (1, H_l, W_l) or None."""
        o, A = ops, self.arena
        half = max(2 * h * w * c for (h, w), c in zip(self.tap_sizes(H, W), (max(ops.LPIPS_CPAD, self.padded[0]),) + self.padded[1:]))
        cur, other = pair_buffers(A, half)
        rows = 2 * H * W
        x = cur[:rows * ops.LPIPS_CPAD].view(rows, ops.LPIPS_CPAD)
        o.lpips_prep(a, x[:H * W], self.affine)
        o.lpips_prep(b, x[H * W:], self.affine)
        j = 0
        for l, idx in enumerate(SLICES):
            for i in idx:
                w, bias = self.w[j]
                y = other[:rows * w.shape[0]].view(rows, w.shape[0])
                o.conv2d(x.view(2, H, W, x.shape[1]), w, y, bias=bias)
                if i != idx[-1]:
                    o.relu_(y)
                x, cur, other, j = y, other, cur, j + 1
            pooled = None
            if l < 4:
                pooled = other[:2 * (H // 2) * (W // 2) * x.shape[1]].view(2 * (H // 2) * (W // 2), x.shape[1])
            o.lpips_tap(x, 1, H, W, self.lin[l], pooled=pooled, dmap=None if maps is None else maps[l], out=out[l])
            if pooled is not None:
                x, cur, other, H, W = pooled, other, cur, H // 2, W // 2
                rows = 2 * H * W

    def __call__(self, a, b, layers=False, spatial=False):
        """LPIPS of `a` against `b`, each what `metrics.psnr` accepts (a PIL image or a list of them, a numpy array, a tensor; 3
        channels, [0, 1] scale or 8-bit).  Returns fp64 (N,) on the device, (N, 5) with `layers` (the five taps' terms, whose sum
        over the row is the score); with `spatial` a pair (that, [five fp32 (N, H_l, W_l) maps of the per-pixel terms])."""
        ta, _ = host_source(a, "a")
        tb, _ = host_source(b, "b")
        da, db = dims(ta), dims(tb)
        if da != db:
            raise ValueError(f"LPIPS: b is (N, C, H, W) = {db} but its counterpart is {da}")
        N, C, H, W = da
        if C != 3:
            raise ValueError(f"LPIPS: a and b must have 3 channels, got {C}")
        self._check_geometry(H, W)
        if self.device.type != "cuda":
            raise ValueError(f"LPIPS: the model was built on {self.device}; there is no host path")
        ta, tb = ta.to(self.device).contiguous(), tb.to(self.device).contiguous()
        res = torch.empty(5, N, dtype=torch.float64, device=self.device)
        maps = [torch.empty(N, h, w, dtype=torch.float32, device=self.device) for h, w in self.tap_sizes(H, W)] if spatial else None
        for n in range(N):
            self._pair(ta[n:n + 1], tb[n:n + 1], H, W, [res[l, n:n + 1] for l in range(5)],
                       None if maps is None else [m[n:n + 1] for m in maps])
        if not bool(torch.isfinite(res).all()):
            raise FloatingPointError(f"LPIPS produced a non-finite tap (activation overflow): this model stores its activations as "
                                     f"{self.dtype_name}; build it with dtype=torch.bfloat16")
        per_layer = res.t().contiguous()
        score = per_layer if layers else per_layer.sum(dim=1)
        return (score, maps) if spatial else score
