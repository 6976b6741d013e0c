"""The VGG-16 trunk LPIPS and DISTS share (DESIGN.md section 7 "The shared VGG-16 pair trunk"): the thirteen 3x3 convs of
torchvision's `features` in five slices, read from either network's state dict, packed for `ops.conv2d`, and walked by one
pair at a time -- the `a` and the `b` image stacked as one batch of two, so that each weight is read once -- between two
activation buffers of one arena.  `PairModel` holds what a scorer on this trunk has in common: construction, the three ways to
build one, the refusals in front of a call, and the walk; after each slice the walk hands the slice's last pre-activation to
the subclass (`instantir_amd.lpips.LPIPS`: the tap; `instantir_amd.dists.DISTS`: the sums and the L2 pool), which returns what
the next slice reads.  Importable without a GPU; there is no host path.
"""
from __future__ import annotations

import torch

from . import ops
from .engine import Arena
from .images import dims, host_source, scoring_device
from .packing import conv_weight_nhwc

CONVS = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)            # torchvision indices of VGG-16 `features`' convs
SLICES = ((0, 2), (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28))  # a halving between slices; each slice's last ReLU is what is scored
VGG_WIDTHS = (64, 128, 256, 512, 512)
MIN_SIDE = 16                                                          # four halvings: the fifth slice keeps one pixel
DTYPES = {torch.float16: "fp16", torch.bfloat16: "bf16"}


def pad64(c):
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


def read_convs(sd, whole, who):
    """The thirteen (weight, bias) pairs in execution order from a state dict: under `whole`, a network's own name rule
    ("net.slice{k}.{i}", "stage{k}.{i}"; k the slice from 1, i the torchvision index), or under torchvision's `features.{i}`
    when `whole` is None.  Each goes through `get_conv`."""
    convs, cin = [], 3
    for k, idx in enumerate(SLICES, 1):
        for i in idx:
            convs.append(get_conv(sd, (whole or "features.{i}").format(k=k, i=i), cin, who))
            cin = convs[-1][0].shape[0]
    return convs


def slice_widths(convs):
    """The output channels of the five slices' last convs."""
    return tuple(convs[j][0].shape[0] for j in (1, 3, 6, 9, 12))


def read_triples(sd, keys, default, who):
    """The optional input normalisation: `default` when `keys[0]` is absent, else the two three-value tuples under `keys`
    (`scaling_layer.shift` / `.scale`, `mean` / `std`) in fp64; another element count raises ValueError naming the key."""
    if keys[0] not in sd:
        return default
    for key in keys:
        if get_tensor(sd, key, who).numel() != 3:
            raise ValueError(f"{who}: {key} must hold 3 values, got {tuple(sd[key].shape)}")
    return tuple(tuple(get_tensor(sd, key, who).double().reshape(3).tolist()) for key in keys)


def load_state_dicts(parse, path, second_path=None):
    """`parse` of one or two files, each read with safetensors or `torch.load(..., weights_only=True)` on the CPU."""
    from .loaders import _load_file
    return parse(_load_file(path), None if second_path is None else _load_file(second_path))


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
        cout = pad64(w.shape[0])
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


def pair_view(buf, H, W, C):
    """The front of `buf` as the (2 H W, C) rows of a stacked pair."""
    return buf[:2 * H * W * C].view(2 * H * W, C)


def check_pair_geometry(who, H, W, nbytes, why):
    """Raised before any launch: a side below MIN_SIDE (`why`); a largest activation of a pair (`nbytes`) of 2 GiB or more, the
    limit of the conv's plain stores."""
    if min(H, W) < MIN_SIDE:
        raise ValueError(f"{who}: the smallest side is {MIN_SIDE} ({why}), got {H}x{W}")
    if nbytes >= 1 << 31:
        raise ValueError(f"{who} of a {H}x{W} pair: its largest activation ({nbytes} bytes) reaches 2 GiB, beyond what the conv "
                         "launches have been verified for; score crops or a smaller size")


class PairModel:
    """A scorer of image pairs on the VGG-16 trunk.  A subclass names itself (`NAME`, `MODULE`, `WHY`: the sentence of the
    smallest-side refusal), lists the channels it scores in front of the five slices (`STAGE0`), binds its module's
    `parse_state_dict` and `synthetic_state_dict`, sets `affine` (what `ops.lpips_prep` reads), and scores in `__call__`."""
    NAME = MODULE = WHY = ""
    STAGE0 = ()
    parse_state_dict = synthetic_state_dict = None

    def __init__(self, convs, device=None, dtype=torch.float16):
        if dtype not in DTYPES:
            raise ValueError(f"{self.NAME}: dtype must be torch.float16 (default) or torch.bfloat16")
        self.device, self.dtype, self.dtype_name = scoring_device(device, self.MODULE), dtype, DTYPES[dtype]
        self.widths = self.STAGE0 + slice_widths(convs)
        self.padded = self.STAGE0 + tuple(pad64(c) for c in slice_widths(convs))      # the conv reads whole 64-channel K tiles (pack_convs)
        self.w = pack_convs(convs, self.device, dtype)
        self.arena = Arena(self.device, dtype)

    @classmethod
    def from_state_dict(cls, sd, second_sd=None, device=None, dtype=torch.float16):
        return cls(*cls.parse_state_dict(sd, second_sd), device=device, dtype=dtype)

    @classmethod
    def from_files(cls, path, second_path=None, device=None, dtype=torch.float16):
        return cls(*load_state_dicts(cls.parse_state_dict, path, second_path), device=device, dtype=dtype)

    @classmethod
    def synthetic(cls, seed, widths=VGG_WIDTHS, device=None, dtype=torch.float16):
        return cls.from_state_dict(cls.synthetic_state_dict(seed, widths), device=device, dtype=dtype)

    # ---- geometry -----------------------------------------------------------------------------------
    def _slice_channels(self):
        """The columns of a pair's rows in each of the five slices; the prepared image is the first slice's floor."""
        c = self.padded[len(self.STAGE0):]
        return (max(ops.LPIPS_CPAD, c[0]),) + c[1:]

    def _largest_activation_bytes(self, H, W):
        return 2 * H * W * self._slice_channels()[0] * 2

    def _check_geometry(self, H, W):
        """Raised before any launch: a side below 16 leaves the fifth slice without a pixel; the largest activation of a pair (both
        images at full resolution in the first slice's channels) must stay below 2 GiB, the limit of the conv's plain stores."""
        check_pair_geometry(self.NAME, H, W, self._largest_activation_bytes(H, W), self.WHY)

    # ---- a call -------------------------------------------------------------------------------------
    def _same_kind(self, ta, tb):
        """The two host sources as the network reads them (as they are, unless a subclass needs them alike)."""
        return ta, tb

    def _upload(self, a, b):
        """The front of a call: `a`, `b` (each what `metrics.psnr` accepts) checked and on the device -> (ta, tb, (N, H, W))."""
        ta, _ = host_source(a, "a")
        tb, _ = host_source(b, "b")
        da, db = dims(ta), dims(tb)
        if da != db:
            raise ValueError(f"{self.NAME}: b is (N, C, H, W) = {db} but its counterpart is {da}")
        N, C, H, W = da
        if C != 3:
            raise ValueError(f"{self.NAME}: a and b must have 3 channels, got {C}")
        self._check_geometry(H, W)
        if self.device.type != "cuda":
            raise ValueError(f"{self.NAME}: the model was built on {self.device}; there is no host path")
        ta, tb = self._same_kind(ta, tb)
        return ta.to(self.device).contiguous(), tb.to(self.device).contiguous(), (N, H, W)

    def _check_finite(self, t, noun):
        if not bool(torch.isfinite(t).all()):
            raise FloatingPointError(f"{self.NAME} produced a non-finite {noun} (activation overflow): this model stores its activations as "
                                     f"{self.dtype_name}; build it with dtype=torch.bfloat16")

    def _trunk(self, a, b, sizes, after_slice):
        """One pair through the thirteen convs: `a`, `b` sources of one image each, `sizes` the (H_l, W_l) of the five slices.
        ReLU follows every conv but a slice's last, whose pre-activation `x` goes to `after_slice(l, x, H, W, other)`: it
        launches what the scorer takes from the slice and returns the next slice's input, a view of `other`, or None."""
        (H, W), chans = sizes[0], self._slice_channels()
        cur, other = pair_buffers(self.arena, max(2 * h * w * c for (h, w), c in zip(sizes, chans)))
        x = pair_view(cur, H, W, ops.LPIPS_CPAD)
        ops.lpips_prep(a, x[:H * W], self.affine)
        ops.lpips_prep(b, x[H * W:], self.affine)
        j = 0
        for l, idx in enumerate(SLICES):
            H, W = sizes[l]
            for i in idx:
                w, bias = self.w[j]
                y = pair_view(other, H, W, w.shape[0])
                ops.conv2d(x.view(2, H, W, x.shape[1]), w, y, bias=bias)
                if i != idx[-1]:
                    ops.relu_(y)
                x, cur, other, j = y, other, cur, j + 1
            x = after_slice(l, x, H, W, other)
            cur, other = other, cur
