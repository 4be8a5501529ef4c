"""Device-framing measurements (DESIGN.md "Device-resident payload framing"): HIP-event times of
shorthair_frame_batch against a device-to-device copy of the same output bytes, and the packet-group
calls with host framing and with device framing.

    python tools/frame_bench.py --out profiles/frame/<tag>.json [--lib <libcauchy256.so>] [--legs kernel,host]

Both legs run 8192 x 200 blocks of B = 1400 on two inputs: "full" (every payload B - 2 bytes) and
"short" (payload lengths uniform in 8..1350, the loopback's traffic).
  kernel  shorthair_frame_batch, 10 back-to-back calls between two HIP events after 40 settle calls,
          three repeats; hipMemcpyAsync device-to-device of the same output bytes timed the same way in
          the same process; bytes written / time and its fraction of the copy's rate
  host    shorthair_encode_groups / shorthair_recover_groups (k = 200, m = 32, on_packet = NULL),
          wall-clock per call and shorthair_groups_traffic bytes per call, on route 0 (host framing)
          and route 1 (device framing). In the short input one payload per group is B - 2 bytes, so
          that the group's block_bytes is 1400 as in the full input.
A library without the framing entry points (the parent commit's build given with --lib) runs the host
leg on its only route, so every library is measured by the same code in one session. ctypes only: the
package's binding is not imported, whichever library is measured.
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
hipMemcpyDeviceToDevice = 3


def load(path):
    lib = C.CDLL(path)
    vp, i, ll = C.c_void_p, C.c_int, C.c_longlong
    lib.shorthair_encode_groups.argtypes = [vp, i]
    lib.shorthair_recover_groups.argtypes = [vp, i, vp, vp]
    lib.cauchy_256_batch_errors.argtypes = [vp]
    lib.has_frame = hasattr(lib, "shorthair_frame_batch")
    if lib.has_frame:
        lib.shorthair_frame_batch.argtypes = [i, i, vp, ll] + [vp] * 5
        lib.shorthair_groups_set_framing.argtypes = [i]
        lib.shorthair_groups_traffic.argtypes = [vp, vp]
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


def lengths(kind, total, rng):
    if kind == "full":
        return np.full(total, B - 2, np.int32)
    return rng.integers(8, 1351, size=total).astype(np.int32)


def leg_kernel(lib, args, res):
    hip = hip_runtime()
    total = args.groups * K
    s = torch.cuda.current_stream().cuda_stream
    out = torch.empty(total * B, dtype=torch.uint8, device="cuda")
    src = torch.randint(0, 256, (total * B,), dtype=torch.uint8, device="cuda")
    r = res["kernel"] = {"blocks": total, "out_bytes": total * B}

    def copy():
        assert hip.hipMemcpyAsync(out.data_ptr(), src.data_ptr(), total * B, hipMemcpyDeviceToDevice, s) == 0

    r["copy_ms"] = [timed(copy, args.iters, args.settle if i == 0 else 3) for i in range(3)]
    copy_gbs = total * B / np.median(r["copy_ms"]) / 1e6
    r["copy_GBps_written"] = copy_gbs
    for kind in ("full", "short"):
        rng = np.random.default_rng(3)
        ln = lengths(kind, total, rng)
        off = np.concatenate([[0], np.cumsum(ln[:-1], dtype=np.int64)]).astype(np.int64)
        pay_bytes = int(off[-1] + ln[-1])
        d_off, d_len = torch.from_numpy(off).cuda(), torch.from_numpy(ln).cuda()
        pay = src[:pay_bytes]  # packed back to back: every alignment occurs

        def frame():
            assert lib.shorthair_frame_batch(B, total, pay.data_ptr(), pay_bytes, d_off.data_ptr(), d_len.data_ptr(),
                                             None, out.data_ptr(), s) == 0

        ms = [timed(frame, args.iters, args.settle if i == 0 else 3) for i in range(3)]
        assert lib.cauchy_256_batch_errors(s) == 0
        # spot check against the rule
        host = out.view(total, B)[[0, 1, total // 2, total - 1]].cpu().numpy()
        for row, j in zip(host, (0, 1, total // 2, total - 1)):
            want = np.zeros(B, np.uint8)
            want[0], want[1] = ln[j] & 0xFF, ln[j] >> 8
            want[2:2 + ln[j]] = src[int(off[j]):int(off[j]) + int(ln[j])].cpu().numpy()
            assert np.array_equal(row, want), j
        gbs = total * B / np.median(ms) / 1e6
        r[kind] = {"payload_bytes": pay_bytes, "frame_ms": ms, "GBps_written": gbs,
                   "fraction_of_copy": gbs / copy_gbs}
        del d_off, d_len


TX = np.dtype([("k", "i4"), ("m", "i4"), ("packets", "u8"), ("lens", "u8"), ("out", "u8"), ("cap", "i4"),
               ("m_out", "i4"), ("stride", "i4")], align=True)
RX = np.dtype([("n_orig", "i4"), ("ids", "u8"), ("data", "u8"), ("lens", "u8"), ("n_rec", "i4"), ("rec", "u8"),
               ("rec_lens", "u8")], align=True)


def traffic(lib):
    if not lib.has_frame:
        return None
    a, b = C.c_longlong(0), C.c_longlong(0)
    lib.shorthair_groups_traffic(C.byref(a), C.byref(b))
    return a.value, b.value


def calls(lib, fn, reps):
    """Wall-clock ms of `reps` calls after one warm call, and the traffic bytes of one call."""
    fn()
    t, t0 = [], traffic(lib)
    for _ in range(reps):
        a = time.perf_counter()
        fn()
        t.append((time.perf_counter() - a) * 1e3)
    t1 = traffic(lib)
    per = None if t0 is None else [(t1[0] - t0[0]) // reps, (t1[1] - t0[1]) // reps]
    return {"ms": t, "h2d_d2h_bytes_per_call": per}


def leg_host(lib, args, res):
    G, total = args.groups, args.groups * K
    res["host"] = {}
    routes = (0, 1) if lib.has_frame else (0,)
    for kind in ("full", "short"):
        rng = np.random.default_rng(5)
        ln = lengths(kind, total, rng).astype(np.int64)
        ln[::K] = B - 2  # every group's block_bytes is B
        off = np.concatenate([[0], np.cumsum(ln[:-1])])
        pay = rng.integers(0, 256, size=int(ln.sum()), dtype=np.uint8)
        ptrs = (pay.ctypes.data + off).astype(np.uint64)
        lens = ln.astype(np.uint16)
        stride = 3 + B
        out = np.zeros(G * M * stride, np.uint8)
        tx = np.zeros(G, TX)
        tx["k"], tx["m"] = K, M
        tx["packets"] = ptrs.ctypes.data + np.arange(G, dtype=np.uint64) * (K * 8)
        tx["lens"] = lens.ctypes.data + np.arange(G, dtype=np.uint64) * (K * 2)
        tx["out"] = out.ctypes.data + np.arange(G, dtype=np.uint64) * (M * stride)
        tx["cap"] = M * stride
        # receiver: every group lost its first M originals and got all M recovery packets
        ids = np.tile(np.arange(M, K, dtype=np.uint8), G)
        keep = (np.arange(total) % K) >= M
        optrs, olens = np.ascontiguousarray(ptrs[keep]), np.ascontiguousarray(lens[keep])
        rptrs = out.ctypes.data + np.arange(G * M, dtype=np.uint64) * stride
        rlens = np.full(G * M, stride, np.int32)
        rx = np.zeros(G, RX)
        rx["n_orig"], rx["n_rec"] = K - M, M
        rx["ids"] = ids.ctypes.data + np.arange(G, dtype=np.uint64) * (K - M)
        rx["data"] = optrs.ctypes.data + np.arange(G, dtype=np.uint64) * ((K - M) * 8)
        rx["lens"] = olens.ctypes.data + np.arange(G, dtype=np.uint64) * ((K - M) * 2)
        rx["rec"] = rptrs.ctypes.data + np.arange(G, dtype=np.uint64) * (M * 8)
        rx["rec_lens"] = rlens.ctypes.data + np.arange(G, dtype=np.uint64) * (M * 4)
        r = res["host"][kind] = {"payload_bytes": int(ln.sum()), "block_bytes_total": total * B}
        first_out = None
        for route in routes:
            if lib.has_frame:
                assert lib.shorthair_groups_set_framing(route) in (0, 1)
            out[:] = 0
            enc = calls(lib, lambda: lib.shorthair_encode_groups(tx.ctypes.data, G) == 0 or sys.exit("encode failed"),
                        args.host_reps)
            if first_out is None:
                first_out = out.copy()
            else:
                assert np.array_equal(out, first_out), "route 1 wire bytes differ from route 0"
            dec = calls(lib, lambda: lib.shorthair_recover_groups(rx.ctypes.data, G, None, None) == G
                        or sys.exit("recover failed"), args.host_reps)
            r["route%d" % route] = {"encode_groups": enc, "recover_groups": dec}
        if lib.has_frame:
            lib.shorthair_groups_set_framing(0)
            for what in ("encode_groups", "recover_groups"):
                r[what + "_route1_over_route0"] = float(np.median(r["route1"][what]["ms"]) /
                                                        np.median(r["route0"][what]["ms"]))
        del pay, out, first_out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--lib", default=os.path.join(ROOT, "shorthair_amd", "libcauchy256.so"))
    p.add_argument("--out", required=True)
    p.add_argument("--groups", type=int, default=8192)
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--settle", type=int, default=40)
    p.add_argument("--host-reps", type=int, default=3)
    p.add_argument("--legs", default="kernel,host")
    args = p.parse_args()
    lib = load(args.lib)
    res = {"lib": os.path.relpath(args.lib, ROOT), "has_frame": lib.has_frame, "k": K, "m": M, "B": B,
           "groups": args.groups, "iters": args.iters, "settle": args.settle, "device": torch.cuda.get_device_name(0)}
    legs = args.legs.split(",")
    if "kernel" in legs and lib.has_frame:
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
