"""Times the wide fields' NTT above 2^16: forward + inverse at rank 2^17, zp880 (L = 14) at batch 16 and
zp440 (L = 7) at batch 32, the batches DESIGN.md 4.2b uses at 2^16.  HIP events on the launch stream
around `iters` fwd+inv steps, after `warmup` steps of the same shape.  Prints one JSON line per field:
ms per step, NTT/s (2 * batch transforms per step) and, where the library reports it, the plan's route.

--lib names the libringo.so to time, so one tree's tool can time another commit's library (a parent
build, where these plans run one launch per stage): the tool binds only the few entry points it calls.
usage: python tools/time_wide_long.py [--lib PATH] [--logn 17] [--iters 20] [--warmup 3] [--label NAME]"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402  (first: libringo then resolves the HIP runtime torch loaded)

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=os.path.join(ROOT, "ringo-snark_amd", "lib", "libringo.so"))
ap.add_argument("--logn", type=int, default=17)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--label", default="")
ap.add_argument("--shapes", default="zp880:16,zp440:32")
args = ap.parse_args()

assert torch.cuda.is_available(), "time_wide_long.py needs the GPU"
vp, u64p = ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)
lib = ctypes.CDLL(args.lib)
lib.rg_field_create.argtypes, lib.rg_field_create.restype = [ctypes.c_int, u64p, ctypes.POINTER(vp)], ctypes.c_int
lib.rg_ntt_create.argtypes, lib.rg_ntt_create.restype = [vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(vp)], ctypes.c_int
for fn in (lib.rg_ntt_fwd_dev, lib.rg_ntt_inv_dev):
    fn.argtypes, fn.restype = [vp, vp, vp, ctypes.c_size_t, vp], ctypes.c_int
lib.rg_last_error.restype = ctypes.c_char_p
has_route = hasattr(lib, "rg_ntt_route_name")
if has_route:
    lib.rg_ntt_route_name.argtypes, lib.rg_ntt_route_name.restype = [vp, ctypes.c_int], ctypes.c_char_p
    lib.rg_ntt_passes.argtypes, lib.rg_ntt_passes.restype = [vp, ctypes.c_int], ctypes.c_int


def ck(st, what):
    if st != 0:
        sys.exit(f"{what}: status {st}: {lib.rg_last_error().decode()}")


FIELDS = json.load(open(os.path.join(ROOT, "tests", "golden", "fields.json")))
N = 1 << args.logn
stream = torch.cuda.Stream()
for shape in args.shapes.split(","):
    name, batch = shape.split(":")
    batch = int(batch)
    q = int(FIELDS[name]["q_hex"], 16)
    L = (q.bit_length() + 63) // 64
    ql = np.array([(q >> (64 * i)) & ((1 << 64) - 1) for i in range(L)], np.uint64)
    f, t = vp(), vp()
    ck(lib.rg_field_create(L, ql.ctypes.data_as(u64p), ctypes.byref(f)), "rg_field_create")
    ck(lib.rg_ntt_create(f, N, 0, ctypes.byref(t)), "rg_ntt_create")  # cyclic: Buckler's embedding transform
    # canonical residues: low limbs uniform, the top limb below q's
    rng = np.random.default_rng(1)
    a = rng.integers(0, 1 << 64, size=(batch * N, L), dtype=np.uint64)
    a[:, L - 1] = rng.integers(0, int(ql[L - 1]), size=batch * N, dtype=np.uint64)
    x = torch.from_numpy(a.view(np.int64).reshape(-1)).cuda()
    y = torch.empty_like(x)
    torch.cuda.synchronize()
    s = stream.cuda_stream

    def step():
        ck(lib.rg_ntt_fwd_dev(t, y.data_ptr(), x.data_ptr(), batch, s), "rg_ntt_fwd_dev")
        ck(lib.rg_ntt_inv_dev(t, y.data_ptr(), y.data_ptr(), batch, s), "rg_ntt_inv_dev")

    with torch.cuda.stream(stream):
        for _ in range(args.warmup):
            step()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        for _ in range(args.iters):
            step()
        t1.record(stream)
    t1.synchronize()
    ms = t0.elapsed_time(t1) / args.iters
    ok = bool((y == x).all().item())  # inv(fwd(x)) == x on the last step
    route = ([lib.rg_ntt_route_name(t, d).decode() + ":" + str(lib.rg_ntt_passes(t, d)) for d in (0, 1)]
             if has_route else None)
    print(json.dumps({"label": args.label, "field": name, "L": L, "logN": args.logn, "batch": batch, "iters": args.iters,
                      "ms_per_step": round(ms, 4), "ntt_per_s": round(2 * batch / ms * 1e3, 1), "route_fwd_inv": route,
                      "roundtrip_ok": ok}), flush=True)
    del x, y
