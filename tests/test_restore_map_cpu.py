"""CPU: the host side of region-selective restoration (`restore_map=`): the per-step threshold table, the noise pair a kept
pixel follows, the checks on a caller's map, the CLI's flags and map lookup, and the new entries' place in the C ABI."""
import ctypes

import numpy as np
import pytest
import torch
from PIL import Image

from instantir_amd import lib, restore_map as rm


# ---- the threshold table ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 6, 30])
def test_threshold_table(n):
    thr = rm.thresholds(n)
    assert len(thr) == n
    assert thr == [(n - 1 - i) / n for i in range(n)]
    assert thr[-1] == 0.0 and all(0.0 <= t < 1.0 for t in thr)
    assert all(a > b for a, b in zip(thr, thr[1:]))                  # a pixel that became free stays free
    t32 = np.asarray(thr, dtype=np.float32)
    assert np.float32(0.0) <= t32[-1]                                # s = 0 is kept on the last step
    assert not (np.float32(1.0) <= t32).any()                        # s = 1 is never kept


@pytest.mark.parametrize("n, want", [(1, {0: 0, 0.3: 1, 0.5: 1, 1: 1}), (6, {0: 0, 0.3: 2, 0.5: 3, 1: 6}),
                                     (30, {0: 0, 0.3: 9, 0.5: 15, 1: 30})])
def test_free_step_count(n, want):
    """s is the fraction of the schedule, from its end, that is free: round-to-nearest-up of s * N steps, the last ones."""
    for s, k in want.items():
        assert rm.free_steps(s, n) == k, (n, s)
        thr = np.asarray(rm.thresholds(n), dtype=np.float32)
        free = ~(np.float32(s) <= thr)
        assert free.sum() == k and free[n - k:].all() and not free[:n - k].any()      # the LAST k steps


def test_thresholds_refuse_an_empty_schedule():
    with pytest.raises(ValueError, match="at least one step"):
        rm.thresholds(0)


# ---- the pair a kept pixel follows --------------------------------------------------------------------------------
def test_keep_pair_is_the_add_noise_pair_of_the_following_entry():
    from instantir_amd.schedulers import (DDIMScheduler, DDPMScheduler, DPMSolverMultistepScheduler,
                                          EulerAncestralDiscreteScheduler, EulerDiscreteScheduler)
    for cls in (DDPMScheduler, DDIMScheduler):
        s = cls()
        s.set_timesteps(6)
        ts = [int(t) for t in s.timesteps]
        for i in range(5):
            acp = s.alphas_cumprod[torch.tensor([ts[i + 1]])]
            assert rm.keep_pair(s, i, ts[i]) == (float((acp ** 0.5)[0]), float(((1 - acp) ** 0.5)[0]))
        assert rm.keep_pair(s, 5, ts[5]) == (1.0, 0.0)
    s = DDPMScheduler()
    s.set_timesteps(timesteps=[900, 500, 20])                        # a caller's timetable: the entry that follows is 500, not t - T/N
    acp = s.alphas_cumprod[torch.tensor([500])]
    assert rm.keep_pair(s, 0, 900) == (float((acp ** 0.5)[0]), float(((1 - acp) ** 0.5)[0]))
    assert rm.keep_pair(s, 2, 20) == (1.0, 0.0)
    for cls in (EulerDiscreteScheduler, EulerAncestralDiscreteScheduler, DPMSolverMultistepScheduler):
        s = cls()
        s.set_timesteps(6)
        for i in range(5):
            assert rm.keep_pair(s, i, float(s.timesteps[i])) == tuple(float(v) for v in s._noise_pair(i + 1))
        assert rm.keep_pair(s, 5, float(s.timesteps[5])) == (1.0, 0.0)


# ---- map validation -----------------------------------------------------------------------------------------------
PX, LAT = (32, 48), (4, 6)


def _prep(m, B=2, nipp=1):
    return rm.prepare(m, B, nipp, PX, LAT, "cpu")


def test_map_forms_and_batch_expansion():
    m2 = torch.rand(*PX)
    out, at_px = _prep(m2)
    assert at_px and out.shape == (2,) + PX and out.dtype == torch.float32 and out.is_contiguous()
    assert torch.equal(out[0], m2) and torch.equal(out[1], m2)       # one map serves the whole batch
    two = torch.rand(2, 1, *LAT)
    out, at_px = _prep(two)
    assert not at_px and torch.equal(out, two[:, 0])
    out, _ = rm.prepare(two, 4, 2, PX, LAT, "cpu")                   # repeated per num_images_per_prompt copy, as lq is
    assert torch.equal(out, two[:, 0].repeat_interleave(2, 0))
    out, _ = _prep(np.full(PX, 0.25, dtype=np.float64))
    assert out.dtype == torch.float32 and float(out.max()) == 0.25
    pil = Image.fromarray((np.arange(PX[0] * PX[1]).reshape(PX) % 256).astype(np.uint8))
    out, at_px = _prep(pil)
    assert at_px and torch.equal(out[0], torch.from_numpy(np.asarray(pil, dtype=np.float32) / 255.0))
    out, _ = _prep([pil, pil.point(lambda v: 255 - v)])
    assert torch.equal(out[1], torch.from_numpy((255 - np.asarray(pil, dtype=np.float32)) / 255.0))
    out, _ = _prep(Image.merge("RGB", [pil] * 3))                    # converted to "L"
    assert out.shape == (2,) + PX


@pytest.mark.parametrize("bad, msg", [
    (torch.full(PX, 1.5), r"must lie in \[0, 1\]"),
    (torch.full(PX, -0.1), r"must lie in \[0, 1\]"),
    (torch.full(PX, float("nan")), "non-finite"),
    (torch.full(PX, float("inf")), "non-finite"),
    (torch.zeros(16, 16), r"must match the image \(32, 48\) or the latent \(4, 6\)"),
    (torch.zeros(3, 1, *PX), "gives 3 maps, the batch has 2"),
    (torch.zeros(2, 3, *PX), r"expected \(H, W\) or \(n, 1, H, W\)"),
    (torch.zeros(5), r"expected \(H, W\) or \(n, 1, H, W\)"),
    ("map.png", "must be a PIL image"),
])
def test_bad_maps_are_refused(bad, msg):
    with pytest.raises(ValueError, match=msg):
        _prep(bad)


@pytest.mark.parametrize("bad", [-1, 2.5, True, 513])
def test_bad_feather_is_refused(bad):
    with pytest.raises(ValueError, match="map_feather"):
        rm.check_feather(bad)


def test_feather_accepts_zero_and_the_default():
    assert rm.check_feather(0) == 0 and rm.check_feather(4) == 4 and rm.check_feather(512) == 512


def test_call_signature_has_the_keywords():
    import inspect
    from instantir_amd.pipeline import InstantIRPipeline, _scalar_row
    sig = inspect.signature(InstantIRPipeline.__call__).parameters
    assert sig["restore_map"].default is None and sig["map_feather"].default == 4
    assert "restore_map" in InstantIRPipeline.__call__.__doc__ and "map_feather" in InstantIRPipeline.__call__.__doc__
    plain, n = _scalar_row(4)
    masked, nm = _scalar_row(4, masked=True)                         # the keep slot follows the default row, which stays as it is
    assert "keep" not in plain and nm == n + 4 and masked["keep"] == slice(n, n + 4)
    assert {k: v for k, v in masked.items() if k != "keep"} == plain


# ---- CLI ----------------------------------------------------------------------------------------------------------
def test_cli_flags():
    from instantir_amd.infer import apply_restore_map, build_parser
    a = build_parser().parse_args(["--test_path", "x"])
    assert a.restore_map is None and a.map_feather == 4
    assert apply_restore_map(a, ["a.png"], (64, 64)) == {}           # without the flag nothing is added to the call
    a = build_parser().parse_args(["--test_path", "x", "--restore_map", "maps", "--map_feather", "0"])
    assert a.restore_map == "maps" and a.map_feather == 0
    with pytest.raises(SystemExit, match="no such file or directory"):
        apply_restore_map(a, ["a.png"], (64, 64))
    a.map_feather = -2
    with pytest.raises(SystemExit, match="--map_feather must be >= 0"):
        apply_restore_map(a, ["a.png"], (64, 64))


def test_cli_map_lookup(tmp_path):
    from instantir_amd.infer import apply_restore_map, build_parser
    one = tmp_path / "one.png"
    Image.fromarray(np.full((10, 20), 255, dtype=np.uint8)).save(one)
    maps = tmp_path / "maps"
    maps.mkdir()
    Image.fromarray(np.full((10, 20), 0, dtype=np.uint8)).save(maps / "a.png")
    Image.fromarray(np.full((10, 20), 128, dtype=np.uint8)).save(maps / "b.png")     # serves the input b.jpg by its stem
    assert rm.map_path_for(str(one), "anything.png") == str(one)     # a file: one map for every input
    assert rm.map_path_for(str(maps), "a.png") == str(maps / "a.png")
    assert rm.map_path_for(str(maps), "b.jpg") == str(maps / "b.png")
    with pytest.raises(FileNotFoundError, match="no map for input c.png"):
        rm.map_path_for(str(maps), "c.png")
    a = build_parser().parse_args(["--test_path", "x", "--restore_map", str(maps), "--map_feather", "2"])
    kw = apply_restore_map(a, ["a.png", "b.jpg"], (64, 32))
    assert kw["map_feather"] == 2 and [m.size for m in kw["restore_map"]] == [(64, 32)] * 2      # resized to the resized input
    assert [m.mode for m in kw["restore_map"]] == ["L", "L"]
    assert np.asarray(kw["restore_map"][0]).max() == 0 and np.asarray(kw["restore_map"][1]).min() == 128
    with pytest.raises(SystemExit, match="no map for input c.png"):
        apply_restore_map(a, ["a.png", "c.png"], (64, 32))


# ---- C ABI --------------------------------------------------------------------------------------------------------
NEW = ("iir_sched_step", "iir_map_pool_max_f32", "iir_region_composite_workspace_bytes", "iir_region_composite_f32")


def test_new_entries_are_declared_bound_and_exported():
    syms = lib.declared_symbols()
    h = ctypes.CDLL(lib.LIB_PATH)
    for s in NEW:
        assert s in syms and s in lib.SIGNATURES and hasattr(h, s), s
    fields = [name for name, _ in lib.SchedDesc._fields_]
    assert all(k in fields for k in ("keep_map", "keep_src", "keep_noise", "keep_coef"))
    header = open(lib.HEADER_PATH).read()
    assert "pipelines/sdxl_instantir.py:1619-1633" in header and ":1388-1403" in header


def test_new_entries_refuse_bad_arguments_without_a_gpu():
    """Validation happens before any HIP call, so it runs without a GPU (pointers are never dereferenced)."""
    h = lib.load()
    P = [4096 + 256 * i for i in range(12)]
    eps, coef, x, prev, kmap, ksrc, knoise, kcoef, hist, eps_out = P[:10]

    def step(**kw):
        a = dict(eps_nhwc=eps, lde=64, B=2, C=4, HW=35, cfg=1, coef=coef, x=x, prev=prev, keep_map=kmap, keep_src=ksrc,
                 keep_noise=knoise, keep_coef=kcoef)
        a.update(kw)
        a.setdefault("groups", lib.STEP_KEEP | (lib.STEP_HIST if a.get("hist") else 0))      # what iir_sched_step_keep implied
        return h.iir_sched_step(ctypes.byref(lib.SchedDesc(**a)), None)

    for k in ("keep_map", "keep_src", "keep_noise", "keep_coef", "eps_nhwc", "coef", "x", "prev"):
        assert step(**{k: None}) == -1, k
    assert step(keep_src=prev) == -1 and step(keep_noise=prev) == -1 # the kept value's sources may not be the output
    assert step(hist=hist, eps_out=eps_out) == -1                    # as the existing entries: no eps_out with a history plane
    assert step(hist=x) == -1 and step(HW=0) == -1
    assert step(groups=0) == -1 and step(keep_map=None, keep_src=None, keep_noise=None, groups=0) == -1     # pointers without the bit
    assert step(groups=lib.STEP_KEEP | 32) == -1                     # a bit outside the four

    pool = lambda H, W, f, src=P[0], dst=P[1]: h.iir_map_pool_max_f32(src, 2, H, W, f, dst, None)
    assert pool(25, 40, 8) == -1 and pool(24, 41, 8) == -1 and pool(24, 40, 0) == -1 and pool(0, 40, 8) == -1
    assert pool(32776, 8, 8) == -1 and pool(24, 40, 8, src=None) == -1 and pool(24, 40, 8, dst=P[0]) == -1

    assert h.iir_region_composite_workspace_bytes(2, 37, 53) == 2 * 37 * 53 * 2
    assert h.iir_region_composite_workspace_bytes(2, 0, 53) == -1 and h.iir_region_composite_workspace_bytes(1, 32769, 8) == -1

    def comp(dec=P[0], orig=P[1], m=P[2], B=2, C=3, H=37, W=53, r=4, ws=P[3], ws_bytes=2 * 37 * 53 * 2, out=P[4]):
        return h.iir_region_composite_f32(dec, orig, m, B, C, H, W, r, ws, ws_bytes, out, None)

    assert comp(r=-1) == -1 and comp(r=513) == -1 and comp(C=0) == -1 and comp(H=0) == -1 and comp(W=32769) == -1
    assert comp(ws_bytes=2 * 37 * 53 * 2 - 1) == -1 and comp(ws=None) == -1 and comp(dec=None) == -1 and comp(m=None) == -1
    assert comp(out=P[1]) == -1 and comp(out=P[2]) == -1 and comp(out=P[3]) == -1     # only `decoded` may be the output
