"""Device-delivery measurements (DESIGN.md "Device-resident delivery of recovered blocks"): HIP-event
times of shorthair_unframe_batch against a device-to-device copy of the same packed bytes, and
shorthair_recover_groups with host delivery and with device delivery on both framing routes.

    python tools/unframe_bench.py --out profiles/unframe/<tag>.json [--lib <libcauchy256.so>] [--legs kernel,host]

  kernel  8192 x 32 slots of B = 1400 (d_out of a k = 200, m = 32 decode) on three inputs: "full" (every
          prefix B - 2), "short" (prefixes uniform in 8..1350) and "sparse" (full prefixes, counts uniform
          in 0..32). shorthair_unframe_batch, 10 back-to-back calls between two HIP events after 40
          settle calls, three repeats; hipMemcpyAsync device-to-device of the same number of packed
          bytes timed the same way in the same process; the ratio of the two rates.
  host    shorthair_recover_groups (k = 200, m = 32, 8192 groups, on_packet = NULL), wall-clock per call
          (three calls after one warm call) and shorthair_groups_traffic bytes per call, framing {0, 1} x
          delivery {0, 1}, on three inputs: "full" and "short" (every group loses 32 originals; in the
          short input one payload per group is B - 2 bytes so that block_bytes is 1400) and "random_e"
          (full payloads, each group loses 1..32 originals).
A library without the delivery entry points (the parent commit's build given with --lib) runs the host
leg with delivery 0 only, so every library is measured by the same code in one session. ctypes only: the
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
    lib.shorthair_groups_set_framing.argtypes = [i]
    lib.shorthair_groups_traffic.argtypes = [vp, vp]
    lib.has_unframe = hasattr(lib, "shorthair_unframe_batch")
    if lib.has_unframe:
        lib.shorthair_unframe_scratch_bytes.argtypes = [i, i]
        lib.shorthair_unframe_scratch_bytes.restype = ll
        lib.shorthair_unframe_batch.argtypes = [i, i, i, ll, vp, vp, vp, ll, vp, vp, vp, vp]
        lib.shorthair_groups_set_delivery.argtypes = [i]
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


def leg_kernel(lib, args, res):
    hip = hip_runtime()
    G, emax = args.groups, M
    slots = G * emax
    s = torch.cuda.current_stream().cuda_stream
    blocks = torch.randint(0, 256, (slots, B), dtype=torch.uint8, device="cuda")
    pay = torch.empty(slots * (B - 2), dtype=torch.uint8, device="cuda")
    d_off = torch.empty(slots + 1, dtype=torch.int64, device="cuda")
    d_len = torch.empty(slots, dtype=torch.int32, device="cuda")
    scratch = torch.empty(lib.shorthair_unframe_scratch_bytes(G, emax), dtype=torch.uint8, device="cuda")
    r = res["kernel"] = {"slots": slots, "block_bytes_total": slots * B}
    for kind in ("full", "short", "sparse"):
        rng = np.random.default_rng(3)
        p = rng.integers(8, 1351, size=slots) if kind == "short" else np.full(slots, B - 2)
        count = rng.integers(0, emax + 1, size=G) if kind == "sparse" else np.full(G, emax)
        pre = torch.from_numpy(np.stack([p & 0xFF, p >> 8], axis=1).astype(np.uint8)).cuda()
        blocks[:, :2] = pre
        d_count = torch.from_numpy(count.astype(np.int32)).cuda()
        live = (np.arange(slots) % emax) < np.repeat(count, emax)
        total = int(p[live].sum())

        def unframe():
            assert lib.shorthair_unframe_batch(B, G, emax, emax, blocks.data_ptr(), d_count.data_ptr(), pay.data_ptr(),
                                               pay.numel(), d_off.data_ptr(), d_len.data_ptr(), scratch.data_ptr(),
                                               s) == 0

        def copy():
            assert hip.hipMemcpyAsync(pay.data_ptr(), blocks.data_ptr(), total, hipMemcpyDeviceToDevice, s) == 0

        copy_ms = [timed(copy, args.iters, args.settle if i == 0 else 3) for i in range(3)]
        ms = [timed(unframe, args.iters, args.settle if i == 0 else 3) for i in range(3)]
        assert lib.cauchy_256_batch_errors(s) == 0
        # spot check against the rule
        off = np.concatenate([[0], np.cumsum(np.where(live, p, 0))])
        assert int(d_off[slots].item()) == total == int(off[-1])
        got_len = d_len.cpu().numpy()
        assert np.array_equal(got_len, np.where(live, p, -1))
        for j in [int(v) for v in np.flatnonzero(live)[[0, 1, live.sum() // 2, -1]]]:
            assert torch.equal(pay[int(off[j]):int(off[j]) + int(p[j])], blocks[j, 2:2 + int(p[j])]), j
        r[kind] = {"packed_bytes": total, "unframe_ms": ms, "copy_ms": copy_ms,
                   "GBps_packed": total / np.median(ms) / 1e6, "copy_GBps": total / np.median(copy_ms) / 1e6,
                   "fraction_of_copy": float(np.median(copy_ms) / np.median(ms))}
        del pre, d_count


TX = np.dtype([("k", "i4"), ("m", "i4"), ("packets", "u8"), ("lens", "u8"), ("out", "u8"), ("cap", "i4"),
               ("m_out", "i4"), ("stride", "i4")], align=True)
RX = np.dtype([("n_orig", "i4"), ("ids", "u8"), ("data", "u8"), ("lens", "u8"), ("n_rec", "i4"), ("rec", "u8"),
               ("rec_lens", "u8")], align=True)


def traffic(lib):
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
    return {"ms": t, "h2d_d2h_bytes_per_call": [(t1[0] - t0[0]) // reps, (t1[1] - t0[1]) // reps]}


def leg_host(lib, args, res):
    G, total = args.groups, args.groups * K
    res["host"] = {}
    deliveries = (0, 1) if lib.has_unframe else (0,)
    for kind in ("full", "short", "random_e"):
        rng = np.random.default_rng(5)
        ln = (rng.integers(8, 1351, size=total) if kind == "short" else np.full(total, B - 2)).astype(np.int64)
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
        assert lib.shorthair_groups_set_framing(0) in (0, 1)
        assert lib.shorthair_encode_groups(tx.ctypes.data, G) == 0
        # receiver: group g lost its first e_g originals and got the first e_g recovery packets
        e = rng.integers(1, M + 1, size=G) if kind == "random_e" else np.full(G, M)
        keep = (np.arange(total) % K) >= np.repeat(e, K)
        ids = np.ascontiguousarray((np.arange(total) % K)[keep].astype(np.uint8))
        optrs, olens = np.ascontiguousarray(ptrs[keep]), np.ascontiguousarray(lens[keep])
        first = np.concatenate([[0], np.cumsum(K - e)[:-1]]).astype(np.uint64)
        rptrs = out.ctypes.data + np.arange(G * M, dtype=np.uint64) * stride
        rlens = np.full(G * M, stride, np.int32)
        rx = np.zeros(G, RX)
        rx["n_orig"], rx["n_rec"] = K - e, e
        rx["ids"] = ids.ctypes.data + first
        rx["data"] = optrs.ctypes.data + first * 8
        rx["lens"] = olens.ctypes.data + first * 2
        rx["rec"] = rptrs.ctypes.data + np.arange(G, dtype=np.uint64) * (M * 8)
        rx["rec_lens"] = rlens.ctypes.data + np.arange(G, dtype=np.uint64) * (M * 4)
        lost = (np.arange(total) % K) < np.repeat(e, K)
        r = res["host"][kind] = {"delivered_payload_bytes": int(ln[lost].sum()), "slots": G * M,
                                 "recovered_blocks": int(e.sum())}
        for framing in (0, 1):
            for delivery in deliveries:
                assert lib.shorthair_groups_set_framing(framing) in (0, 1)
                if lib.has_unframe:
                    assert lib.shorthair_groups_set_delivery(delivery) in (0, 1)
                r["framing%d_delivery%d" % (framing, delivery)] = calls(
                    lib, lambda: lib.shorthair_recover_groups(rx.ctypes.data, G, None, None) == G
                    or sys.exit("recover failed"), args.host_reps)
        lib.shorthair_groups_set_framing(0)
        if lib.has_unframe:
            lib.shorthair_groups_set_delivery(0)
            for framing in (0, 1):
                r["framing%d_delivery1_over_delivery0" % framing] = float(
                    np.median(r["framing%d_delivery1" % framing]["ms"]) /
                    np.median(r["framing%d_delivery0" % framing]["ms"]))
        del pay, out


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
    res = {"lib": os.path.relpath(args.lib, ROOT), "has_unframe": lib.has_unframe, "k": K, "m": M, "B": B,
           "groups": args.groups, "iters": args.iters, "settle": args.settle, "device": torch.cuda.get_device_name(0)}
    legs = args.legs.split(",")
    if "kernel" in legs and lib.has_unframe:
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
