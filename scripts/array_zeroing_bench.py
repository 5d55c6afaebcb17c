"""What does the zeroing in front of an array-response launch cost?  Two hipMemsetAsync calls, back to back on the null stream, of
nr * nt planes of 1024 x 1024 fp32 each (re and im of a 1 x 1, 2 x 2, 4 x 4 and 8 x 8 matrix at configs[1]'s grid), HIP events around
30 pairs, the median of 4 blocks and the blocks' range.  Nothing of the library is loaded: the HIP runtime through ctypes.
DESIGN.md K3-M subtracts these figures from scripts/array_response_bench.py's.

    python scripts/array_zeroing_bench.py [--out profiles/array_zeroing_bench.txt]
"""
import argparse
import ctypes as C
import os
import statistics

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "array_zeroing_bench.txt"))
args = ap.parse_args()
lines = []

try:
    hip = C.CDLL("libamdhip64.so")
except OSError:
    hip = C.CDLL("/opt/rocm/lib/libamdhip64.so")
hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
hip.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
hip.hipEventSynchronize.argtypes = [C.c_void_p]
hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
hip.hipFree.argtypes = [C.c_void_p]


def ok(rc):
    if rc != 0:
        raise SystemExit(f"HIP call failed with {rc}")


ok(hip.hipSetDevice(0))
e0, e1 = C.c_void_p(), C.c_void_p()
ok(hip.hipEventCreate(C.byref(e0)))
ok(hip.hipEventCreate(C.byref(e1)))
plane = 1024 * 1024 * 4
for pairs in (1, 4, 16, 64):
    size = pairs * plane
    a, b = C.c_void_p(), C.c_void_p()
    ok(hip.hipMalloc(C.byref(a), size))
    ok(hip.hipMalloc(C.byref(b), size))
    for _ in range(5):
        ok(hip.hipMemsetAsync(a, 0, size, None))
        ok(hip.hipMemsetAsync(b, 0, size, None))
    ok(hip.hipDeviceSynchronize())
    ms = []
    for _ in range(4):
        ok(hip.hipEventRecord(e0, None))
        for _ in range(30):
            ok(hip.hipMemsetAsync(a, 0, size, None))
            ok(hip.hipMemsetAsync(b, 0, size, None))
        ok(hip.hipEventRecord(e1, None))
        ok(hip.hipEventSynchronize(e1))
        t = C.c_float()
        ok(hip.hipEventElapsedTime(C.byref(t), e0, e1))
        ms.append(t.value / 30)
    lines.append(f"{pairs} pairs: two memsets of {size >> 20} MiB: {statistics.median(ms):.4f} ms (blocks {min(ms):.4f} .. {max(ms):.4f})")
    print(lines[-1], flush=True)
    ok(hip.hipFree(a))
    ok(hip.hipFree(b))
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
