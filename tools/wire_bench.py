"""Wire-emit measurements (DESIGN.md "Device-resident wire packets"): HIP-event times of
shorthair_wire_emit_batch against a device-to-device copy of the same output bytes, the cost of the
separate launch behind an encode, and shorthair_encode_groups with the packets built on the host and on
the GPU.

    python tools/wire_bench.py --out profiles/wire/<tag>.json [--lib <libcauchy256.so>] [--legs kernel,host]

Shape: 8192 groups, m = 32, B = 1400, k = 200 (var: k_g uniform in 120..200).
  kernel  shorthair_wire_emit_batch, uniform and var-k, into a 16-byte-aligned d_wire and one 5 bytes
          past it: 10 back-to-back calls between two HIP events after 40 settle calls, three repeats;
          hipMemcpyAsync device-to-device of the same groups * m * (3 + B) bytes timed the same way in
          the same process; then cauchy_256_encode_batch alone and encode + emit on one stream.
  host    shorthair_encode_groups, wall-clock per call and shorthair_groups_traffic bytes per call, on
          "full" (every payload B - 2 bytes) and "short" (lengths uniform in 8..1350, one B - 2 per
          group) inputs, framing 0 and 1, wire 0 and 1, --reps repetitions of --host-calls calls per
          leg with the legs interleaved; a repetition's figure is the median of its calls.
A library without the wire entry points (the parent commit's build given with --lib) runs the host legs
on wire 0 alone, so both libraries are measured by the same code in one session: run the two
alternately, a process each. ctypes only: the package's binding is not imported, whichever library is
measured.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
K, M, B = 200, 32, 1400
KMIN = 120
S = 3 + B
hipMemcpyDeviceToDevice = 3


def load(path):
    lib = C.CDLL(path)
    vp, i = C.c_void_p, C.c_int
    lib.shorthair_encode_groups.argtypes = [vp, i]
    lib.cauchy_256_encode_batch.argtypes = [i] * 4 + [vp] * 3
    lib.cauchy_256_batch_errors.argtypes = [vp]
    lib.shorthair_groups_set_framing.argtypes = [i]
    lib.shorthair_groups_traffic.argtypes = [vp, vp]
    lib.has_wire = hasattr(lib, "shorthair_wire_emit_batch")
    if lib.has_wire:
        lib.shorthair_wire_emit_batch.argtypes = [i] * 4 + [vp, i] + [vp] * 3
        lib.shorthair_groups_set_wire.argtypes = [i]
    assert lib.cauchy_256_batch_init(0) == 0
    return lib


def hip_runtime():
    """The HIP runtime this process already has (torch's): the same file, so the same copy."""
    for line in open("/proc/self/maps"):
        path = line.split()[-1]
        if os.path.basename(path).startswith("libamdhip64.so"):
            hip = C.CDLL(path)
            hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
            return hip
    raise RuntimeError("no libamdhip64 loaded")


def timed(fn, iters, settle):
    """Mean ms of fn() over `iters` back-to-back runs between two HIP events, after `settle` runs."""
    for _ in range(settle):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def repeats(fn, args):
    return [timed(fn, args.iters, args.settle if i == 0 else 3) for i in range(3)]


def check_records(wire, rec, ks, G):
    """A few records against the rule, from the device arrays."""
    for p in (0, 1, M - 1, M, (G // 2) * M + 7, G * M - 1):
        g, y = divmod(p, M)
        got = wire[p * S:(p + 1) * S].cpu().numpy()
        want = np.concatenate([[ks[g] + y, ks[g] - 1, M - 1], rec[p * B:(p + 1) * B].cpu().numpy()]).astype(np.uint8)
        assert np.array_equal(got, want), p


def leg_kernel(lib, args, res):
    hip = hip_runtime()
    G = args.groups
    n_in, n_out = G * M * B, G * M * S
    s = torch.cuda.current_stream().cuda_stream
    rec = torch.randint(0, 256, (n_in,), dtype=torch.uint8, device="cuda")
    src = torch.randint(0, 256, (n_out,), dtype=torch.uint8, device="cuda")
    buf = torch.empty(n_out + 16, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0 and rec.data_ptr() % 16 == 0
    r = res["kernel"] = {"records": G * M, "in_bytes": n_in, "out_bytes": n_out}

    def copy():
        assert hip.hipMemcpyAsync(buf.data_ptr(), src.data_ptr(), n_out, hipMemcpyDeviceToDevice, s) == 0

    r["copy_ms"] = repeats(copy, args)
    copy_ms = float(np.median(r["copy_ms"]))
    r["copy_GBps_written"] = n_out / copy_ms / 1e6
    rng = np.random.default_rng(3)
    ks_var = rng.integers(KMIN, K + 1, size=G)
    first = np.concatenate([[0], np.cumsum(ks_var)]).astype(np.int32)
    d_first = torch.from_numpy(first).cuda()
    for name, dfirst, total, ks in (("uniform", None, 0, np.full(G, K)), ("var", d_first.data_ptr(), int(first[-1]), ks_var)):
        for mis in (0, 5):
            wire = buf[mis:mis + n_out]

            def emit():
                assert lib.shorthair_wire_emit_batch(K, M, B, G, dfirst, total, rec.data_ptr(), wire.data_ptr(), s) == 0

            ms = repeats(emit, args)
            check_records(wire, rec, ks, G)
            med = float(np.median(ms))
            r["%s_align%d" % (name, mis)] = {"emit_ms": ms, "GBps_written": n_out / med / 1e6,
                                             "copy_over_emit": copy_ms / med}
    assert lib.cauchy_256_batch_errors(s) == 0
    del src
    # the separate launch: encode alone against encode + emit on the same stream
    data = torch.randint(0, 256, (G * K * B,), dtype=torch.uint8, device="cuda")
    wire = buf[:n_out]

    def encode():
        assert lib.cauchy_256_encode_batch(K, M, B, G, data.data_ptr(), rec.data_ptr(), s) == 0

    def encode_emit():
        encode()
        assert lib.shorthair_wire_emit_batch(K, M, B, G, None, 0, rec.data_ptr(), wire.data_ptr(), s) == 0

    # alternated, so that a drift of the clocks falls on both
    enc, both = [], []
    for i in range(3):
        enc.append(timed(encode, args.iters, args.settle if i == 0 else 3))
        both.append(timed(encode_emit, args.iters, 3))
    check_records(wire, rec, np.full(G, K), G)
    r["separate_launch"] = {"encode_ms": enc, "encode_emit_ms": both,
                            "difference_ms": float(np.median(both) - np.median(enc))}


TX = np.dtype([("k", "i4"), ("m", "i4"), ("packets", "u8"), ("lens", "u8"), ("out", "u8"), ("cap", "i4"),
               ("m_out", "i4"), ("stride", "i4")], align=True)


def traffic(lib):
    a, b = C.c_longlong(0), C.c_longlong(0)
    lib.shorthair_groups_traffic(C.byref(a), C.byref(b))
    return a.value, b.value


def lengths(kind, total, rng):
    if kind == "full":
        return np.full(total, B - 2, np.int64)
    return rng.integers(8, 1351, size=total).astype(np.int64)


def leg_host(lib, args, res):
    G, total = args.groups, args.groups * K
    res["host"] = {}
    legs = [(f, w) for f in (0, 1) for w in ((0, 1) if lib.has_wire else (0,))]
    for kind in ("full", "short"):
        rng = np.random.default_rng(5)
        ln = lengths(kind, total, rng)
        ln[::K] = B - 2  # every group's block_bytes is B
        off = np.concatenate([[0], np.cumsum(ln[:-1])])
        pay = rng.integers(0, 256, size=int(ln.sum()), dtype=np.uint8)
        ptrs = (pay.ctypes.data + off).astype(np.uint64)
        lens = ln.astype(np.uint16)
        out = np.zeros(G * M * S, np.uint8)
        tx = np.zeros(G, TX)
        tx["k"], tx["m"] = K, M
        tx["packets"] = ptrs.ctypes.data + np.arange(G, dtype=np.uint64) * (K * 8)
        tx["lens"] = lens.ctypes.data + np.arange(G, dtype=np.uint64) * (K * 2)
        tx["out"] = out.ctypes.data + np.arange(G, dtype=np.uint64) * (M * S)
        tx["cap"] = M * S
        r = res["host"][kind] = {"payload_bytes": int(ln.sum()), "block_bytes_total": total * B, "legs": {}}
        first_out = None
        for rep in range(args.reps + 1):  # repetition 0 warms every leg (and checks its bytes) untimed
            for framing, wire in legs:
                l, name = lib, "framing%d_wire%d" % (framing, wire)
                assert l.shorthair_groups_set_framing(framing) in (0, 1)
                if l.has_wire:
                    assert l.shorthair_groups_set_wire(wire) in (0, 1)
                if rep == 0:
                    out[:] = 0
                    assert l.shorthair_encode_groups(tx.ctypes.data, G) == 0
                    if first_out is None:
                        first_out = out.copy()
                    assert np.array_equal(out, first_out), name + ": wire bytes differ"
                    r["legs"][name] = {"rep_ms": [], "calls_ms": []}
                    continue
                t, t0 = [], traffic(l)
                for _ in range(args.host_calls):
                    a = time.perf_counter()
                    assert l.shorthair_encode_groups(tx.ctypes.data, G) == 0
                    t.append((time.perf_counter() - a) * 1e3)
                t1 = traffic(l)
                leg = r["legs"][name]
                leg["calls_ms"].append(t)
                leg["rep_ms"].append(float(np.median(t)))
                leg["h2d_d2h_bytes_per_call"] = [(t1[0] - t0[0]) // args.host_calls, (t1[1] - t0[1]) // args.host_calls]
        lib.shorthair_groups_set_framing(0)
        if lib.has_wire:
            lib.shorthair_groups_set_wire(0)
        for name, leg in r["legs"].items():
            leg["median_ms"] = float(np.median(leg["rep_ms"]))
            leg["min_ms"], leg["max_ms"] = float(min(leg["rep_ms"])), float(max(leg["rep_ms"]))
        del pay, out, first_out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--lib", default=os.path.join(ROOT, "shorthair_amd", "libcauchy256.so"))
    p.add_argument("--out", required=True)
    p.add_argument("--groups", type=int, default=8192)
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--settle", type=int, default=40)
    p.add_argument("--reps", type=int, default=1)
    p.add_argument("--host-calls", type=int, default=3)
    p.add_argument("--legs", default="kernel,host")
    args = p.parse_args()
    lib = load(args.lib)
    res = {"lib": os.path.relpath(args.lib, ROOT), "has_wire": lib.has_wire,
           "k": K, "kmin_var": KMIN, "m": M, "B": B, "groups": args.groups, "iters": args.iters, "settle": args.settle,
           "reps": args.reps, "host_calls": args.host_calls, "device": torch.cuda.get_device_name(0)}
    legs = args.legs.split(",")
    if "kernel" in legs and lib.has_wire:
        leg_kernel(lib, args, res)
        torch.cuda.empty_cache()
    if "host" in legs:
        leg_host(lib, args, res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    sys.exit(main())
