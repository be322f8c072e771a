"""A/B of the 4-limb NTT above 2^16: the long Fast256 route (ntt256_edge_pass + ntt256_pass over 2^16-point blocks,
three passes) against the generic tiled route (ntt_pass_kernel<4, P>, two passes) on q255 (jindo_zp) and zp220,
forward + inverse, cyclic (Buckler's embedding transform), at 2^17 x 32, 2^18 x 16, 2^19 x 8 and batch 1
of each rank.

Both legs run the experiments library (libringo_exp.so), each in child processes of their own: the default
route, and RINGO_NTT_KERNEL=r, which keeps these plans on the tiled route the library used before the long
route existed.  The children of the two legs alternate, `--repeats` times each; a child times every shape
with HIP events on its launch stream around `--iters` fwd+inv steps after `--warmup` steps of the same
shape, and checks inv(fwd(x)) == x on the last one.  The parent process never touches the GPU.

Output: one JSON line per (field, logN, batch) with each leg's (`default`: no switch; `r`) median, min and
max ms per step over the repeats, and the verdict of the routing rule: the long route wins a shape when its
median is below the tiled median by more than the spread (the larger max - min of the two legs).

--lib names the library to time, so this tool can time another commit's build (with --legs default there:
its own route, tiled before the long route existed, to confirm that the r leg here is that commit's time).
usage: python tools/time_fast256_long.py [--lib PATH] [--repeats 3] [--iters 10] [--warmup 2] [--legs default,r]"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(17, 32), (18, 16), (19, 8), (17, 1), (18, 1), (19, 1)]
FIELD_NAMES = ["jindo_zp", "zp220"]

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=os.path.join(ROOT, "ringo-snark_amd", "lib", "libringo_exp.so"))
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--legs", default="default,r")
ap.add_argument("--child-timeout", type=int, default=240)
ap.add_argument("--child", action="store_true", help="(internal) time every shape in this process")
args = ap.parse_args()


def child():
    import numpy as np
    import torch  # first: the library then resolves the HIP runtime torch loaded

    assert torch.cuda.is_available(), "time_fast256_long.py needs the GPU"
    vp, u64p = ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)
    lib = ctypes.CDLL(args.lib)
    lib.rg_field_create.argtypes, lib.rg_field_create.restype = [ctypes.c_int, u64p, ctypes.POINTER(vp)], ctypes.c_int
    lib.rg_ntt_create.argtypes, lib.rg_ntt_create.restype = [vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(vp)], ctypes.c_int
    lib.rg_ntt_destroy.argtypes = [vp]
    for fn in (lib.rg_ntt_fwd_dev, lib.rg_ntt_inv_dev):
        fn.argtypes, fn.restype = [vp, vp, vp, ctypes.c_size_t, vp], ctypes.c_int
    lib.rg_last_error.restype = ctypes.c_char_p
    lib.rg_ntt_route_name.argtypes, lib.rg_ntt_route_name.restype = [vp, ctypes.c_int], ctypes.c_char_p
    lib.rg_ntt_passes.argtypes, lib.rg_ntt_passes.restype = [vp, ctypes.c_int], ctypes.c_int

    def ck(st, what):
        if st != 0:
            sys.exit(f"{what}: status {st}: {lib.rg_last_error().decode()}")

    fields = json.load(open(os.path.join(ROOT, "tests", "golden", "fields.json")))
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    for name in FIELD_NAMES:
        q = int(fields[name]["q_hex"], 16)
        L = 4
        ql = np.array([(q >> (64 * i)) & ((1 << 64) - 1) for i in range(L)], np.uint64)
        f = vp()
        ck(lib.rg_field_create(L, ql.ctypes.data_as(u64p), ctypes.byref(f)), "rg_field_create")
        plans = {}
        for logn, batch in SHAPES:
            N = 1 << logn
            if logn not in plans:
                plans[logn] = vp()
                ck(lib.rg_ntt_create(f, N, 0, ctypes.byref(plans[logn])), "rg_ntt_create")
            t = plans[logn]
            rng = np.random.default_rng(logn)  # canonical residues: the top limb below q's
            a = rng.integers(0, 1 << 64, size=(batch * N, L), dtype=np.uint64)
            a[:, L - 1] = rng.integers(0, int(ql[L - 1]), size=batch * N, dtype=np.uint64)
            x = torch.from_numpy(a.view(np.int64).reshape(-1)).cuda()
            y = torch.empty_like(x)
            torch.cuda.synchronize()

            def step():
                ck(lib.rg_ntt_fwd_dev(t, y.data_ptr(), x.data_ptr(), batch, s), "rg_ntt_fwd_dev")
                ck(lib.rg_ntt_inv_dev(t, y.data_ptr(), y.data_ptr(), batch, s), "rg_ntt_inv_dev")

            iters = args.iters * (8 if batch == 1 else 1)  # a window of comparable length
            with torch.cuda.stream(stream):
                for _ in range(args.warmup):
                    step()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record(stream)
                for _ in range(iters):
                    step()
                t1.record(stream)
            t1.synchronize()
            ms = t0.elapsed_time(t1) / iters
            ok = bool((y == x).all().item())
            route = [lib.rg_ntt_route_name(t, d).decode() + ":" + str(lib.rg_ntt_passes(t, d)) for d in (0, 1)]
            print(json.dumps({"field": name, "logN": logn, "batch": batch, "iters": iters, "ms_per_step": round(ms, 4),
                              "route_fwd_inv": route, "roundtrip_ok": ok}), flush=True)
            del x, y
        for t in plans.values():
            lib.rg_ntt_destroy(t)


def parent():
    legs = args.legs.split(",")
    times, routes = {}, {}
    for rep in range(args.repeats):
        for leg in legs:
            env = dict(os.environ)
            env.pop("RINGO_NTT_KERNEL", None)
            if leg != "default":
                env["RINGO_NTT_KERNEL"] = leg
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--lib", args.lib, "--iters", str(args.iters),
                   "--warmup", str(args.warmup)]
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.child_timeout)
            if r.returncode != 0:
                sys.exit(f"child ({leg}, repeat {rep}) failed with {r.returncode}: {r.stderr[-2000:]}")
            print(f"repeat {rep} leg {leg}: done", file=sys.stderr, flush=True)
            for line in r.stdout.splitlines():
                if not line.startswith("{"):
                    continue
                d = json.loads(line)
                if not d["roundtrip_ok"]:
                    sys.exit(f"child ({leg}): inv(fwd(x)) != x at {d}")
                key = (d["field"], d["logN"], d["batch"])
                times.setdefault(key, {}).setdefault(leg, []).append(d["ms_per_step"])
                routes.setdefault(key, {})[leg] = d["route_fwd_inv"]
    for key in sorted(times):
        out = {"field": key[0], "logN": key[1], "batch": key[2], "repeats": args.repeats, "lib": os.path.basename(args.lib)}
        for leg, v in times[key].items():
            out[leg] = {"median_ms": round(statistics.median(v), 4), "min_ms": min(v), "max_ms": max(v),
                        "ntt_per_s": round(2 * key[2] / statistics.median(v) * 1e3, 1), "route_fwd_inv": routes[key][leg]}
        if "default" in times[key] and "r" in times[key]:
            a, b = times[key]["default"], times[key]["r"]
            spread = max(max(a) - min(a), max(b) - min(b))
            out["spread_ms"] = round(spread, 4)
            out["speedup"] = round(statistics.median(b) / statistics.median(a), 3)
            out["long_wins"] = statistics.median(a) < statistics.median(b) - spread
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    child() if args.child else parent()
