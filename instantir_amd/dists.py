"""DISTS (Ding et al., "Image Quality Assessment: Unifying Structure and Texture Similarity", TPAMI 2020; VGG-16) on the device:
the full-reference figure restoration papers report beside LPIPS, scored on restored images like `metrics.lpips` (DESIGN.md
section 7 "DISTS").  The reference has no counterpart.

    from instantir_amd.dists import DISTS
    model = DISTS.from_files("vgg16.pth", "weights.pt", device="cuda:0")     # torchvision VGG-16 + DISTS's alpha / beta
    model = DISTS.from_files("dists_full.pth", device="cuda:0")              # or one whole DISTS state dict
    model(restored, gt)                       # fp64 (N,) on the device; components=True: + (N, 6, 2) structure / texture terms

The contract.  Stage 0 is the raw image x itself (fp32, never rounded to a 16-bit type).  The trunk reads h = (x - mean) / std
(`ops.lpips_prep` with shift = 2 mean - 1, scale = 2 std); stage 1 is convs 0, 2 of VGG-16 `features`, stages 2 to 5 apply L2
pooling to the stage before (`ops.dists_l2pool`: sqrt of the Hann-weighted 3x3 stride-2 blur of the squares, + 1e-12, output
sides ceil(H / 2), ceil(W / 2)) and then convs (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28); a ReLU follows every conv
(`ops.relu_`, or on read inside the two DISTS kernels).  The `a` and the `b` image of a pair run stacked as one batch of two,
so each weight is read once.  Of each of the 3 + 64 + 128 + 256 + 512 + 512 = 1475 channels `ops.dists_stats` /
`ops.dists_image_stats` give {sum a, sum b, sum a^2, sum b^2, sum ab} over the stage's n pixels in fp64; from them, in torch
fp64 on the device:  mu = sum / n,  s_a^2 = E[a^2] - mu_a^2,  s_ab = E[ab] - mu_a mu_b,
    S1 = (2 mu_a mu_b + c1) / (mu_a^2 + mu_b^2 + c1),   S2 = (2 s_ab + c2) / (s_a^2 + s_b^2 + c2),   c1 = c2 = 1e-6,
    DISTS = 1 - sum_c (alpha_c S1_c + beta_c S2_c) / (sum alpha + sum beta).
Pairs are processed one at a time from one activation arena, so memory does not grow with the batch.  There is no host path.

No real DISTS weights exist offline: the two file formats are read as the packages write them to the best of public
knowledge, and `DISTS.synthetic` / `synthetic_state_dict` draw seeded stand-ins the CPU restatement of the tests rebuilds.
"""
from __future__ import annotations

import torch

from . import ops
from .vgg import VGG_WIDTHS, PairModel, get_tensor, load_state_dicts, pair_view, read_convs, read_triples, slice_widths, synthetic_convs

STAGES = 6
C1 = C2 = 1e-6
MEAN, STD = ops.DISTS_MEAN, ops.DISTS_STD
WHO = "DISTS weights"


def synthetic_state_dict(seed, widths=VGG_WIDTHS):
    """A whole DISTS state dict (format (b) of `parse_state_dict`) of seeded fp32 CPU tensors: the convs and biases drawn as
    `lpips.synthetic_state_dict` draws them, then alpha and beta uniform in [0, 1), each (1, 3 + sum(widths), 1, 1)."""
    g = torch.Generator()
    g.manual_seed(int(seed))
    sd, widths = synthetic_convs(g, widths, lambda k, i: f"stage{k}.{i}", "DISTS")
    chns = 3 + sum(widths)
    sd["alpha"] = torch.rand(1, chns, 1, 1, generator=g)
    sd["beta"] = torch.rand(1, chns, 1, 1, generator=g)
    return sd


def parse_state_dict(sd, weights_sd=None):
    """-> (convs, alpha, beta, mean, std): thirteen (weight (Cout, Cin, 3, 3), bias (Cout,)) pairs in execution order, alpha and
    beta as fp64 (3 + sum of the stage widths,), and the input normalisation, all on the CPU.  Two formats, told apart by their
    keys:
      (a) a torchvision VGG-16 state dict (`features.{i}.weight` / `.bias`) plus `weights_sd`, DISTS's `weights.pt` (`alpha`,
          `beta`, each shaped (1, 1475, 1, 1));
      (b) a whole DISTS state dict: `stage{k}.{i}.weight` / `.bias` with the same i, `alpha`, `beta`, optional `mean` / `std`
          (the `stage{k}.{i}.filter` buffers of its L2 pools are ignored: the Hann window is the contract's).
    Widths come from the tensors.  A missing key, a kernel that is not 3x3, a width that is not a multiple of 8, a channel count
    that does not follow from the layer before and an alpha / beta of another length raise ValueError naming the key."""
    whole = any(k.startswith("stage") for k in sd)
    src = sd if whole else weights_sd
    if src is None:
        raise ValueError(f"{WHO}: a torchvision VGG-16 state dict needs alpha and beta too (weights_path: DISTS's weights.pt, "
                         "keys alpha, beta)")
    convs, vecs = read_convs(sd, "stage{k}.{i}" if whole else None, WHO), []
    chns = 3 + sum(slice_widths(convs))
    for key in ("alpha", "beta"):
        v = get_tensor(src, key, WHO)
        if v.numel() != chns or tuple(v.shape) not in ((1, chns, 1, 1), (chns,)):
            raise ValueError(f"{WHO}: {key} must be shaped (1, {chns}, 1, 1), got {tuple(v.shape)}")
        vecs.append(v.double().reshape(chns).contiguous())
    mean, std = read_triples(sd if whole else {}, ("mean", "std"), (MEAN, STD), WHO)
    return convs, vecs[0], vecs[1], mean, std


def load_weights(path, weights_path=None):
    """`parse_state_dict` of one or two files, each read with safetensors or `torch.load(..., weights_only=True)` on the CPU."""
    return load_state_dicts(parse_state_dict, path, weights_path)


class DISTS(PairModel):
    """`from_state_dict(sd, weights_sd)`, `from_files(vgg_or_dists_path, weights_path)` and `synthetic(seed, widths)` build one."""
    NAME, MODULE, WHY = "DISTS", "instantir_amd.dists", "as for LPIPS: four halvings must leave the last stage a pixel"
    STAGE0 = (3,)                                                             # stage 0 is the image: `widths` and `padded` start with it
    parse_state_dict, synthetic_state_dict = staticmethod(parse_state_dict), staticmethod(synthetic_state_dict)

    def __init__(self, convs, alpha, beta, mean=MEAN, std=STD, device=None, dtype=torch.float16):
        super().__init__(convs, device, dtype)
        # the sums of a pair: one row per (padded) channel, stage after stage.  Padding channels carry a = b = 0, which gives
        # S = 1, so the weighting gathers the real channels only: (STAGES, widest) indices, the tail of a narrower stage
        # pointing at its first channel with weight 0.
        self.offsets = tuple(sum(self.padded[:k]) for k in range(STAGES + 1))
        widest = max(self.widths)
        idx = torch.zeros(STAGES, widest, dtype=torch.long)
        wa, wb = torch.zeros(STAGES, widest, dtype=torch.float64), torch.zeros(STAGES, widest, dtype=torch.float64)
        alpha, beta, at = alpha.double().reshape(-1), beta.double().reshape(-1), 0
        if alpha.numel() != sum(self.widths) or beta.numel() != sum(self.widths):
            raise ValueError(f"DISTS: alpha and beta must hold {sum(self.widths)} values, got {alpha.numel()} and {beta.numel()}")
        for k, c in enumerate(self.widths):
            idx[k] = self.offsets[k]
            idx[k, :c] = self.offsets[k] + torch.arange(c)
            wa[k, :c], wb[k, :c] = alpha[at:at + c], beta[at:at + c]
            at += c
        total = float(alpha.sum() + beta.sum())
        if not total > 0.0:
            raise ValueError("DISTS: alpha and beta must sum to a positive weight")
        self.index = idx.to(self.device)
        self.alpha, self.beta = (wa / total).to(self.device), (wb / total).to(self.device)
        self.mean, self.std = tuple(mean), tuple(std)
        self.affine = ops.dists_affine(self.device, mean, std)
        self.ws = None

    def stage_sizes(self, H, W):
        """(H_k, W_k) of the six stages: the image twice, then ceil halving by each of the four L2 pools."""
        sizes = [(H, W), (H, W)]
        for _ in range(4):
            H, W = (H + 1) // 2, (W + 1) // 2
            sizes.append((H, W))
        return sizes

    def _workspace(self, H, W):
        need = max([ops.dists_image_stats_workspace_bytes(1, H, W)]
                   + [ops.dists_stats_workspace_bytes(1, h, w, c) for (h, w), c in zip(self.stage_sizes(H, W)[1:], self.padded[1:])])
        if self.ws is None or self.ws.numel() * 8 < need:
            self.ws = torch.empty((need + 7) // 8, dtype=torch.float64, device=self.device)
        return self.ws

    # ---- the network --------------------------------------------------------------------------------
    def _pair(self, a, b, H, W, sums):
        """One pair through the network: a, b sources of one image each (the same kind); sums: fp64 (offsets[-1], 5)."""
        sizes, ws = self.stage_sizes(H, W)[1:], self._workspace(H, W)
        out = lambda k: sums[self.offsets[k]:self.offsets[k + 1]].view(1, self.padded[k], ops.DISTS_STATS)
        ops.dists_image_stats(a, b, ws=ws, out=out(0))

        def stage(l, x, H, W, other):
            ops.dists_stats(x, 1, H, W, ws=ws, out=out(l + 1))
            return ops.dists_l2pool(x, 2, H, W, out=pair_view(other, *sizes[l + 1], x.shape[1])) if l < 4 else None
        self._trunk(a, b, sizes, stage)

    def _same_kind(self, ta, tb):
        """Stage 0 reads both sources as one kind: of a mixed pair the uint8 one becomes its fp32 copy, u / 255 in fp32 (on the
        host: a division)."""
        if ta.dtype != tb.dtype:
            ta, tb = (t.permute(0, 3, 1, 2).float() / 255.0 if t.dtype == torch.uint8 else t for t in (ta, tb))
        return ta, tb

    def _terms(self, sums, pixels):
        """fp64 (STAGES, 2): the structure and the texture term of every stage from a pair's sums; their sum is 1 - DISTS."""
        s = sums[self.index] / pixels                                         # (STAGES, widest, 5): the means of a, b, a^2, b^2, ab
        mu_a, mu_b = s[..., 0], s[..., 1]
        var_a, var_b, cov = s[..., 2] - mu_a * mu_a, s[..., 3] - mu_b * mu_b, s[..., 4] - mu_a * mu_b
        s1 = (2.0 * mu_a * mu_b + C1) / (mu_a * mu_a + mu_b * mu_b + C1)
        s2 = (2.0 * cov + C2) / (var_a + var_b + C2)
        return torch.stack([(self.alpha * s1).sum(dim=1), (self.beta * s2).sum(dim=1)], dim=1)

    def __call__(self, a, b, components=False):
        """DISTS of `a` against `b`, each what `metrics.psnr` accepts (a PIL image or a list of them, a numpy array, a tensor; 3
        channels, [0, 1] scale or 8-bit).  Returns fp64 (N,) on the device; with `components` a pair (that, fp64 (N, 6, 2): per
        stage the structure term sum_c alpha_c S1_c / ws and the texture term sum_c beta_c S2_c / ws, whose sum is 1 - score)."""
        ta, tb, (N, H, W) = self._upload(a, b)
        pixels = torch.tensor([float(h * w) for h, w in self.stage_sizes(H, W)], dtype=torch.float64).view(STAGES, 1, 1).to(self.device)
        sums = torch.empty(N, self.offsets[-1], ops.DISTS_STATS, dtype=torch.float64, device=self.device)
        terms = torch.empty(N, STAGES, 2, dtype=torch.float64, device=self.device)
        for n in range(N):
            self._pair(ta[n:n + 1], tb[n:n + 1], H, W, sums[n])
            terms[n] = self._terms(sums[n], pixels)
        self._check_finite(sums, "sum")
        score = torch.stack([1.0 - terms[n].sum() for n in range(N)])
        return (score, terms) if components else score
