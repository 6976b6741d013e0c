"""The launch trace of the three encoder towers, recorded on a CPU with `ops` replaced by a recording object.

    python tests/golden/make_encoder_trace.py <commit id of the recording checkout> [path]

`replay()` builds the towers of tests/golden/encoder_cases.py with device="cpu" and swaps the `ops` that
instantir_amd/encoders.py sees for a `Recorder`.  The recorder keeps the `ACT_*` constants and, for every launch (`gemm`,
`layernorm`, `attention`, `copy_add`), feeds a SHA-256 with the op name and every argument after binding it to the real
wrapper's signature (so a default and the same value passed explicitly are one launch): a tensor's shape, strides, dtype and
bytes, a scalar's value, the K / V^T segment list element by element.  The launch's output operand (`out`, `out`, `o`, `dst`)
enters with its geometry only -- its bytes are what `torch.empty` left -- and is then filled, through the view the launch
was given, with values derived from that digest.  A later launch that reads another buffer, the same buffer at another time,
or another slice of it therefore gets another digest: the trace pins the order of the launches, their operand geometry, their
scalar arguments and where every operand came from.  Per case the golden holds the digests (8 bytes each), the op names, and
the digest of what the call returned.

Nothing here depends on the CPU that records: every weight and pixel is a small integer (|v| <= 4), so the LayerScale and
value-bias folds, the concatenations and the fp16 casts of the weight packing are exact in any summation order; only native
position tables are used (no bicubic resize); no activation function is evaluated.

The committed encoder_trace.npz was written on the tree whose instantir_amd/encoders.py was still that of the parent of the
commit that gave the three towers one block packer and one block loop (its id is stored under `PARENT_KEY`), after two
replays that agreed.  tests/test_encoder_trace_cpu.py replays on the current code and names the first launch that differs.
"""
import functools
import hashlib
import inspect
import os
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "encoder_trace.npz")
PARENT_KEY = "recorded_by_commit"


class Recorder:
    OUT = {"gemm": "out", "layernorm": "out", "attention": "o", "copy_add": "dst"}     # the operand each launch writes

    def __init__(self, real):
        self.real, self.launches = real, []

    def __getattr__(self, name):
        if name in self.OUT:
            return functools.partial(self._launch, name)
        value = getattr(self.real, name)
        if callable(value):
            raise AttributeError(f"instantir_amd.encoders launches ops.{name}, which the trace recorder does not know")
        return value

    def _feed(self, h, v, geometry_only=False):
        import torch
        if torch.is_tensor(v):
            h.update(repr((tuple(v.shape), v.stride(), str(v.dtype))).encode())
            if not geometry_only:
                h.update(v.contiguous().view(torch.uint8).numpy().tobytes())
        elif isinstance(v, (list, tuple)):
            h.update(b"[")
            for e in v:
                self._feed(h, e)
            h.update(b"]")
        elif isinstance(v, float):
            h.update(struct.pack("<d", v))
        elif v is None or isinstance(v, (bool, int)):
            h.update(repr(v).encode())
        else:
            raise TypeError(f"trace recorder: argument of type {type(v).__name__}")

    def _launch(self, name, *args, **kwargs):
        import torch
        bound = inspect.signature(getattr(self.real, name)).bind(*args, **kwargs)
        bound.apply_defaults()
        h = hashlib.sha256(name.encode())
        for pname, v in bound.arguments.items():
            h.update(pname.encode())
            self._feed(h, v, geometry_only=pname == self.OUT[name])
        digest = h.digest()
        out = bound.arguments[self.OUT[name]]
        if name == "copy_add":
            off = bound.arguments["dst_off"]
            out = out[:, off:off + bound.arguments["src"].shape[1]]
        fill = np.frombuffer(hashlib.shake_256(digest).digest(out.numel()), dtype=np.uint8).astype(np.float32)
        out.copy_(torch.from_numpy((fill - 128.0) / 64.0).view(out.shape))            # multiples of 1/64 in [-2, 2): exact in fp16
        self.launches.append((name, digest[:8]))
        return bound.arguments[self.OUT[name]]


def replay():
    """{case: (op names, digests (n, 8) uint8, digest of the returned tensors (32,) uint8)}"""
    import torch
    sys.path[:0] = [p for p in (os.path.dirname(os.path.dirname(HERE)), HERE) if p not in sys.path]
    import encoder_cases as EC
    from instantir_amd import encoders
    rec = Recorder(encoders.ops)
    out = {}
    encoders.ops = rec
    try:
        for case, call in EC.cases(EC.draw_ints, "cpu", native_only=True):
            rec.launches = []
            h = hashlib.sha256()
            for name, t in call().items():
                h.update(name.encode())
                rec._feed(h, t)
            assert case not in out, case
            out[case] = ([n for n, _ in rec.launches], np.frombuffer(b"".join(d for _, d in rec.launches), dtype=np.uint8).reshape(-1, 8),
                         np.frombuffer(h.digest(), dtype=np.uint8))
    finally:
        encoders.ops = rec.real
    return out


def first_difference(got, want_launches, want_returned):
    """None, or a sentence naming the first launch of one case that differs from the recorded one."""
    names, launches, returned = got
    for i in range(min(len(launches), len(want_launches))):
        if not np.array_equal(launches[i], want_launches[i]):
            return f"launch {i} ({names[i]}) differs: its op, an operand's geometry or bytes, or a scalar argument"
    if len(launches) != len(want_launches):
        return f"{len(launches)} launches, {len(want_launches)} recorded"
    if not np.array_equal(returned, want_returned):
        return "every launch matches, but the returned tensors differ"
    return None


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    path = sys.argv[2] if len(sys.argv) > 2 else PATH
    trace, again = replay(), replay()
    differ = [c for c in trace if first_difference(again[c], trace[c][1], trace[c][2])]
    if differ or sorted(trace) != sorted(again):
        sys.exit(f"two recordings differ: {differ}")
    store = {PARENT_KEY: np.frombuffer(sys.argv[1].encode(), dtype=np.uint8)}
    for case, (names, launches, returned) in trace.items():
        store[case + "/ops"] = np.frombuffer(",".join(names).encode(), dtype=np.uint8)
        store[case + "/launches"], store[case + "/returned"] = launches, returned
    np.savez_compressed(path, **store)
    print(f"wrote {path}: {len(trace)} cases, {sum(len(v[1]) for v in trace.values())} launches recorded twice by {sys.argv[1]}, "
          f"{os.path.getsize(path)} bytes")
