"""Bits of the per-step latent update, recorded through the exported C entries (pack, CFG rescale, scheduler step).

    python tests/golden/make_sched_update_bits.py          # on an MI355X: writes tests/golden/sched_update_bits.npz

`replay()` drives iir_sched_step and iir_cfg_rescale_factor (plain, PAG, HIST and PAG | HIST descriptors; the keys keep the names
of the positional entries that once spelled those forms, as labels), iir_sched_step{,_hist}_f32 and
iir_pack_latent_t / iir_pack_latent_dscale through `lib.load()` on seeded inputs and returns every output buffer as an
integer view: the full array at (B, H, W) = (2, 5, 7) (70 threads: one partial block, odd HW), its SHA-256 digest at
(2, 16, 16) (512 threads: two blocks).  The committed file was written by the library as it stood before the scheduler-update
kernels were folded into one per family; tests/test_sigma_schedulers_gpu.py replays the calls on the current library and
asserts equality, so any change of the update's bits (or a host path that swaps prev / x0_out / hist) shows.

    python tests/golden/make_sched_update_bits.py --keep-apg   # writes tests/golden/sched_update_bits_keep_apg.npz

`replay_keep_apg()` does the same for the restore-map and APG forms, through ops.sched_step / ops.apg_project.  That file was
written by the library as it stood before the step's positional entries were replaced by the descriptor entry.
"""
import ctypes
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "sched_update_bits.npz")
PATH_KEEP_APG = os.path.join(HERE, "sched_update_bits_keep_apg.npz")

C, LDE = 4, 8
SHAPES = {"small": (2, 5, 7), "large": (2, 16, 16)}
# {g, sb, sa, k_x0, k_x, k_eps, k_noise, k_h}: every term on (the entries without a history plane ignore [7])
COEF = [6.5, 0.93, 0.37, 0.41, 0.98, 0.12, 0.07, -0.031]
PAG_S, PHI, PACK_SCALE, FILL = 2.75, 0.7, 0.0862, 7.0
KEEP_COEF = [0.5, 0.8, 0.6, 0.0]          # {thr, a, b, 0}: both terms of the kept value on
APG_PAR = [0.3, 2.5, -0.5, 0.0]           # {eta, r, beta_t, 0}: beta_t != 0 (apg_avg is read), r below ||A|| (the clamp engages)


def _record(out, key, t, full):
    a = t.detach().cpu().contiguous().numpy()
    a = a.view({2: np.int16, 4: np.int32}[a.dtype.itemsize])
    out[key] = a if full else np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8)


def replay():
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from instantir_amd import lib
    h = lib.load()
    dev = torch.device("cuda:0")
    out = {}
    for tag, (B, H, W) in SHAPES.items():
        full = tag == "small"
        HW = H * W
        rng = np.random.RandomState(1000 * B + HW)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        eps16 = up(rng.standard_normal((3 * B * HW, LDE)).astype(np.float16))          # uncond | cond | perturbed rows
        x = up((rng.standard_normal((B, C, H, W)) * 3).astype(np.float32))
        noise = up(rng.standard_normal((B, C, H, W)).astype(np.float32))
        m_prev = up(rng.standard_normal((B, C, H, W)).astype(np.float32))
        e32 = up(rng.standard_normal((B, C, H, W)).astype(np.float32))
        fac_in = up(np.array([0.8, 1.3], dtype=np.float32))
        coef = up(np.array(COEF, dtype=np.float32))
        ps = up(np.array([PAG_S], dtype=np.float32))
        scale = up(np.array([PACK_SCALE], dtype=np.float32))
        new = lambda: torch.full((B, C, H, W), FILL, dtype=torch.float32, device=dev)
        p = lambda t: None if t is None else t.data_ptr()

        for hist_on in (False, True):
            for pag in (False, True):
                for cfg in (0, 1):
                    for nz in (False, True):
                        name = "iir_sched_step" + ("_hist" if hist_on else "") + ("_pag" if pag else "")
                        key = f"{tag}.{name}.cfg{cfg}.noise{int(nz)}"
                        prev, x0, eo, hist = new(), new(), new(), m_prev.clone()
                        fac = fac_in if cfg else None
                        # without CFG the eps rows are [cond | perturbed]: start at the cond rows of the buffer
                        e = eps16 if cfg else eps16[B * HW:]
                        d = lib.SchedDesc(eps_nhwc=e.data_ptr(), lde=LDE, B=B, C=C, HW=HW, cfg=cfg, coef=coef.data_ptr(), x=x.data_ptr(),
                                          noise=p(noise if nz else None), prev=prev.data_ptr(), x0_out=x0.data_ptr(), eps_factor=p(fac),
                                          groups=(lib.STEP_HIST if hist_on else 0) | (lib.STEP_PAG if pag else 0),
                                          pag_scale=p(ps if pag else None), hist=p(hist if hist_on else None),
                                          eps_out=p(None if hist_on else eo))
                        rc = h.iir_sched_step(ctypes.byref(d), None)
                        torch.cuda.synchronize()
                        assert rc == 0, (key, rc)
                        _record(out, key + ".prev", prev, full)
                        _record(out, key + ".x0_out", x0, full)
                        _record(out, key + (".hist" if hist_on else ".eps_out"), hist if hist_on else eo, full)

        for pag in (False, True):
            name = "iir_cfg_rescale_factor" + ("_pag" if pag else "")
            f = torch.full((B,), FILL, dtype=torch.float32, device=dev)
            d = lib.SchedDesc(eps_nhwc=eps16.data_ptr(), lde=LDE, B=B, C=C, HW=HW, coef=coef.data_ptr(),
                              groups=lib.STEP_PAG if pag else 0, pag_scale=p(ps if pag else None))
            rc = h.iir_cfg_rescale_factor(ctypes.byref(d), PHI, f.data_ptr(), None)
            torch.cuda.synchronize()
            assert rc == 0, (name, rc)
            _record(out, f"{tag}.{name}.factor", f, True)

        n = B * C * HW
        for nz in (False, True):
            prev, x0 = new(), new()
            rc = h.iir_sched_step_f32(e32.data_ptr(), x.data_ptr(), p(noise if nz else None), coef.data_ptr(), n, prev.data_ptr(),
                                      x0.data_ptr(), None)
            torch.cuda.synchronize()
            assert rc == 0, ("iir_sched_step_f32", rc)
            _record(out, f"{tag}.iir_sched_step_f32.noise{int(nz)}.prev", prev, full)
            _record(out, f"{tag}.iir_sched_step_f32.noise{int(nz)}.x0_out", x0, full)
            prev, x0, hist = new(), new(), m_prev.clone()
            rc = h.iir_sched_step_hist_f32(e32.data_ptr(), x.data_ptr(), p(noise if nz else None), coef.data_ptr(), hist.data_ptr(), n,
                                           prev.data_ptr(), x0.data_ptr(), None)
            torch.cuda.synchronize()
            assert rc == 0, ("iir_sched_step_hist_f32", rc)
            _record(out, f"{tag}.iir_sched_step_hist_f32.noise{int(nz)}.prev", prev, full)
            _record(out, f"{tag}.iir_sched_step_hist_f32.noise{int(nz)}.x0_out", x0, full)
            _record(out, f"{tag}.iir_sched_step_hist_f32.noise{int(nz)}.hist", hist, full)

        rep = 2
        for dt, dtype in ((0, torch.float16), (1, torch.bfloat16)):          # IIR_DT_F16, IIR_DT_BF16
            a =torch.full((rep * B * HW, LDE), FILL, dtype=dtype, device=dev)
            b = a.clone()
            rc = h.iir_pack_latent_t(x.data_ptr(), B, C, HW, a.data_ptr(), LDE, rep, PACK_SCALE, dt, None)
            rc2 = h.iir_pack_latent_dscale(x.data_ptr(), B, C, HW, b.data_ptr(), LDE, rep, scale.data_ptr(), dt, None)
            torch.cuda.synchronize()
            assert rc == 0 and rc2 == 0, ("pack", rc, rc2)
            _record(out, f"{tag}.iir_pack_latent_t.dtype{dt}.out", a.view(torch.int16), full)
            _record(out, f"{tag}.iir_pack_latent_dscale.dtype{dt}.out", b.view(torch.int16), full)
    return out


def replay_keep_apg():
    """The restore-map and APG forms of the step, through ops.sched_step / ops.apg_project (the spelling that did not change
    when the exported entries did): keep x {hist} x {pag} x {cfg}, and apg x {keep} x {hist}."""
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from instantir_amd import ops
    dev = torch.device("cuda:0")
    out = {}
    for tag, (B, H, W) in SHAPES.items():
        full = tag == "small"
        HW = H * W
        rng = np.random.RandomState(77000 + 1000 * B + HW)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        plane = lambda s=1.0: up((rng.standard_normal((B, C, H, W)) * s).astype(np.float32))
        eps16 = up(rng.standard_normal((3 * B * HW, LDE)).astype(np.float16))          # uncond | cond | perturbed rows
        x, noise, m_prev, src, noise0, a_prev = plane(3), plane(), plane(), plane(2), plane(), plane(2)
        kmap = rng.uniform(0, 1, (B, HW)).astype(np.float32)                           # pixels on both sides of thr ...
        kmap[:, ::5] = KEEP_COEF[0]                                                    # ... and on it (kept: map <= thr)
        keep = (up(kmap), src, noise0, up(np.array(KEEP_COEF, dtype=np.float32)))
        fac_in = up(np.array([0.8, 1.3], dtype=np.float32))
        coef = up(np.array(COEF, dtype=np.float32))
        ps = up(np.array([PAG_S], dtype=np.float32))
        par = up(np.array(APG_PAR, dtype=np.float32))
        new = lambda: torch.full((B, C, H, W), FILL, dtype=torch.float32, device=dev)

        def step(key, e, cfg, hist_on, **kw):
            prev, x0, eo, hist = new(), new(), new(), m_prev.clone()
            outs = dict(hist=hist) if hist_on else dict(eps_out=eo)
            ops.sched_step(e, B, coef, x, prev, noise=noise, cfg=bool(cfg), x0_out=x0, **outs, **kw)
            torch.cuda.synchronize()
            _record(out, key + ".prev", prev, full)
            _record(out, key + ".x0_out", x0, full)
            _record(out, key + (".hist" if hist_on else ".eps_out"), hist if hist_on else eo, full)

        for hist_on in (False, True):
            for pag in (False, True):
                for cfg in (0, 1):
                    # without CFG the eps rows are [cond | perturbed]: start at the cond rows of the buffer
                    step(f"{tag}.keep.hist{int(hist_on)}.pag{int(pag)}.cfg{cfg}", eps16 if cfg else eps16[B * HW:], cfg, hist_on,
                         keep=keep, pag_scale=ps if pag else None, eps_factor=fac_in if cfg else None)

        ws = ops.apg_workspace(B, dev)
        for keep_on in (False, True):
            for hist_on in (False, True):
                key = f"{tag}.apg.keep{int(keep_on)}.hist{int(hist_on)}"
                apg = (a_prev.clone(), torch.full((2 * B,), FILL, dtype=torch.float32, device=dev), par)
                ops.apg_project(eps16, B, coef, x, apg, ws)
                step(key, eps16, 1, hist_on, keep=keep if keep_on else None, apg=apg)
                _record(out, key + ".apg_avg", apg[0], full)
                _record(out, key + ".apg_sa", apg[1], True)
    return out


if __name__ == "__main__":
    keep_apg = sys.argv[1:2] == ["--keep-apg"]
    argv = sys.argv[2:] if keep_apg else sys.argv[1:]
    path = argv[0] if argv else (PATH_KEEP_APG if keep_apg else PATH)
    bits = replay_keep_apg() if keep_apg else replay()
    np.savez_compressed(path, **bits)
    print(f"wrote {path}: {len(bits)} buffers, {os.path.getsize(path)} bytes")
