"""Device resampling (ops.resample) cost on one MI355X, beside the PIL call each launch pair replaces.

    python tools/resample_bench.py [--iters 200]

The product's three shapes, one 3-channel 8-bit image each, quantised mode (PIL's arithmetic):
    512 x 384 -> 1024 x 768 bilinear      (resize_img to the working size)
    1024^2 -> 256^2, crop 224, bicubic    (the image encoders' preprocessing, normalisation fused)
    1024^2 -> 2048^2 Lanczos              (the resize back to a large requested output)
per shape: the launches from an uploaded uint8 image and from fp32 planar, by device events, warm, best of two alternating
windows of `--iters` calls; an empty launch (iir_resample_pass on a 1 x 1 image) the same way; the byte floor from the shapes
(source read once, intermediate written and read once, result written once; the tables are not counted) over 6.29 TB/s; and
the host time of the PIL call it replaces (`Image.resize`, plus crop / float conversion / normalisation for the
preprocessing shape, and the upload either form needs), medians of `--host-iters` calls.

    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/resample_bench.py --kernels 50

launches only the HIP kernels, `--kernels` times per shape, for a per-kernel time table."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_TBS = 6.29
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
# (in (H, W), out (H, W), filter, window or None)
SHAPES = [((384, 512), (768, 1024), "bilinear", None),
          ((1024, 1024), (256, 256), "bicubic", (16, 16, 224, 224)),
          ((1024, 1024), (2048, 2048), "lanczos", None)]


def timed(fn, n):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def floor_bytes(in_hw, out_hw, window, src_bytes):
    (H, W), (oh, ow) = in_hw, out_hw
    y0, x0, h, w = window or (0, 0, oh, ow)
    src = 3 * H * W * src_bytes
    mid = 3 * H * w * 4 if (H != oh and W != ow) else 0
    return src + 2 * mid + 3 * h * w * 4


def host_call(im, out_hw, flt, window):
    """The PIL form of one shape, as the product's host path runs it (encoders.dinov2_preprocess for the windowed shape)."""
    r = im.resize((out_hw[1], out_hw[0]), flt)
    if window is None:
        return r
    y0, x0, h, w = window
    arr = np.asarray(r.crop((x0, y0, x0 + w, y0 + h)), dtype=np.float32) / 255.0
    return torch.from_numpy(((arr - np.array(MEAN, dtype=np.float32)) / np.array(STD, dtype=np.float32))[None]).permute(0, 3, 1, 2).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--host-iters", type=int, default=9)
    ap.add_argument("--kernels", type=int, default=0, help="only launch the HIP kernels this many times (for rocprofv3)")
    args = ap.parse_args()
    from PIL import Image
    from instantir_amd import lib, ops
    lib.load()
    if not torch.cuda.is_available():
        raise SystemExit("resample_bench needs an MI355X: there is nothing to time on the host")
    dev = torch.device("cuda:0")
    pil_filter = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}
    one, one_out = torch.zeros(1, 1, 1, 3, dtype=torch.uint8, device=dev), torch.empty(1, 3, 1, 1, device=dev)
    for in_hw, out_hw, flt, window in SHAPES:
        u8 = np.random.default_rng(in_hw[0]).integers(0, 256, (1,) + in_hw + (3,), dtype=np.uint8)
        s_u8 = torch.from_numpy(u8).to(dev)
        s_f32 = s_u8.permute(0, 3, 1, 2).float().contiguous()
        opt = dict(quantize=True, window=window)
        if window is not None:
            opt.update(scale=[1 / (255 * s) for s in STD], bias=[-m / s for m, s in zip(MEAN, STD)])
        out = torch.empty((1, 3) + (tuple(window[2:]) if window else out_hw), device=dev)
        legs = {"uint8": lambda: ops.resample(s_u8, out_hw, flt, out=out, **opt), "fp32": lambda: ops.resample(s_f32, out_hw, flt, out=out, **opt),
                "empty": lambda: ops.resample(one, (1, 1), flt, quantize=True, out=one_out)}
        tag = f"{in_hw[1]}x{in_hw[0]} -> {out_hw[1]}x{out_hw[0]} {flt}{' crop %d' % window[2] if window else ''}"
        if args.kernels:
            timed(legs["uint8"], args.kernels)
            timed(legs["fp32"], args.kernels)
            continue
        us = {k: 1e30 for k in legs}
        for _ in range(2):
            for k, fn in legs.items():
                us[k] = min(us[k], timed(fn, args.iters))
        im = Image.fromarray(u8[0])
        host = []
        for _ in range(args.host_iters):
            t0 = time.perf_counter()
            r = host_call(im, out_hw, pil_filter[flt], window)
            host.append((time.perf_counter() - t0) * 1e6)
        f32_host = r if torch.is_tensor(r) else torch.from_numpy(np.asarray(r, dtype=np.float32))
        up = {"f32": [], "u8": []}
        for _ in range(args.host_iters):
            for k, t in (("f32", f32_host), ("u8", torch.from_numpy(u8))):
                t0 = time.perf_counter()
                t.to(dev)
                torch.cuda.synchronize()
                up[k].append((time.perf_counter() - t0) * 1e6)
        upload_f32, upload_u8 = statistics.median(up["f32"]), statistics.median(up["u8"])
        passes = 2 if (in_hw[0] != out_hw[0] and in_hw[1] != out_hw[1]) else 1
        for k, sb in (("uint8", 1), ("fp32", 4)):
            fb = floor_bytes(in_hw, out_hw, window, sb)
            fl = fb / (HBM_TBS * 1e12) * 1e6
            net = us[k] - passes * us["empty"]
            net_txt = f"{100 * fl / net:.0f} % net of {passes} empty launches" if net > 1.0 else f"no more than {passes} empty launches cost: issue-bound"
            print(f"{tag:44s} {k:5s}: {us[k]:7.1f} us for {passes} launches (empty launch {us['empty']:.1f} us), byte floor {fb / 1e6:.1f} MB = "
                  f"{fl:.1f} us ({100 * fl / us[k]:.0f} % of it reached; {net_txt})", flush=True)
        print(f"{tag:44s} host : PIL {statistics.median(host):.0f} us median of {args.host_iters} (min {min(host):.0f}), its fp32 upload "
              f"{upload_f32:.0f} us; the uint8 upload of the device form {upload_u8:.0f} us (medians)", flush=True)


if __name__ == "__main__":
    main()
