"""Var-k batch measurements (DESIGN.md "Var-k batches"): HIP-event times of the var-k calls against
the uniform calls, after the same settle steps bench.py uses.

    python tools/var_bench.py --out profiles/var/<tag>.json [--lib <libcauchy256.so>] [--legs ...]

Legs (all at m = 32, B = 1400, 8192 groups unless --groups):
  headline  every k_g = 200: uniform encode / decode three times (the box's run-to-run spread),
            then the var calls on the same blocks (their outputs must equal the uniform calls')
  mixed     k_g uniform in 120..200: one var launch against one uniform call per distinct k over
            the same groups (the only option without the var calls)
  host      the mixed workload through shorthair_encode_groups / shorthair_recover_groups
            (on_packet = NULL), wall-clock
A library without the var-k entry points (an older build given with --lib) runs the uniform parts
only, so both libraries are measured by the same code in one session. ctypes only: the package's
binding is not imported, whichever library is measured.
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
M, B = 32, 1400


def load(path):
    lib = C.CDLL(path)
    vp, i = C.c_void_p, C.c_int
    lib.cauchy_256_encode_batch.argtypes = [i] * 4 + [vp] * 3
    lib.cauchy_256_decode_batch_out.argtypes = [i] * 4 + [vp] * 6
    lib.cauchy_256_batch_reserve.argtypes = [i] * 4
    lib.cauchy_256_batch_errors.argtypes = [vp]
    lib.cauchy_256_fill_synthetic.argtypes = [vp, i, i, i, C.c_ulonglong, C.c_ulonglong, vp]
    lib.cauchy_256_erasure_pattern.argtypes = [C.c_ulonglong, i, i, C.c_ulonglong, i, vp]
    lib.has_var = hasattr(lib, "cauchy_256_encode_batch_var")
    if lib.has_var:
        lib.cauchy_256_encode_batch_var.argtypes = [i] * 4 + [vp, i] + [vp] * 3
        lib.cauchy_256_decode_batch_out_var.argtypes = [i] * 4 + [vp, i] + [vp] * 6
    lib.shorthair_encode_groups.argtypes = [vp, i]
    lib.shorthair_recover_groups.argtypes = [vp, i, vp, vp]
    assert lib.cauchy_256_batch_init(0) == 0
    return lib


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


class Batch:
    """A packed batch of groups with k_g = ks[g]: inputs, recovery blocks and decode inputs that lose
    m originals per group (survivors ascending, then the m recovery rows), built on the GPU."""

    def __init__(self, lib, ks, encode):
        self.ks = np.asarray(ks, np.int32)
        G = self.G = len(ks)
        self.first_np = np.concatenate([[0], np.cumsum(self.ks)]).astype(np.int32)
        total = self.total = int(self.first_np[-1])
        self.first = torch.from_numpy(self.first_np).cuda()
        self.data = torch.empty((total, B), dtype=torch.uint8, device="cuda")
        s = torch.cuda.current_stream().cuda_stream
        assert lib.cauchy_256_fill_synthetic(self.data.data_ptr(), 1, B, total, 0, 0xBE, s) == 0
        self.rec = torch.zeros((G, M, B), dtype=torch.uint8, device="cuda")
        encode(self)
        torch.cuda.synchronize()
        rows = np.zeros(total, np.uint8)
        idx = np.zeros(total, np.int64)
        buf = np.zeros(256, np.uint8)
        for g in range(G):
            k, f = int(self.ks[g]), int(self.first_np[g])
            e = lib.cauchy_256_erasure_pattern(g, k, M, 0xBE, M, buf.ctypes.data)
            assert e == M
            r = buf[:k].astype(np.int64)
            rows[f:f + k] = buf[:k]
            idx[f:f + k] = np.where(r < k, f + r, total + g * M + (r - k))
        self.rows = torch.from_numpy(rows).cuda()
        whole = torch.cat([self.data, self.rec.view(G * M, B)])
        self.blocks = whole[torch.from_numpy(idx).cuda()].contiguous()
        del whole
        self.out = torch.zeros((G, M, B), dtype=torch.uint8, device="cuda")
        self.out_rows = torch.zeros((G, M), dtype=torch.uint8, device="cuda")
        self.cnt = torch.zeros(G, dtype=torch.int32, device="cuda")


def uniform_calls(lib, b, what):
    """One uniform call per run of equal k in b.ks (b sorted by k: one call per distinct k)."""
    s = torch.cuda.current_stream().cuda_stream
    g = 0
    while g < b.G:
        k = int(b.ks[g])
        n = 1
        while g + n < b.G and b.ks[g + n] == k:
            n += 1
        f = int(b.first_np[g])
        if what == "enc":
            rc = lib.cauchy_256_encode_batch(k, M, B, n, b.data.data_ptr() + f * B, b.rec.data_ptr() + g * M * B, s)
        else:
            rc = lib.cauchy_256_decode_batch_out(k, M, B, n, b.blocks.data_ptr() + f * B, b.rows.data_ptr() + f,
                                                 b.out.data_ptr() + g * M * B, b.out_rows.data_ptr() + g * M,
                                                 b.cnt.data_ptr() + 4 * g, s)
        assert rc == 0
        g += n


def var_call(lib, b, what, kmax):
    s = torch.cuda.current_stream().cuda_stream
    if what == "enc":
        rc = lib.cauchy_256_encode_batch_var(kmax, M, B, b.G, b.first.data_ptr(), b.total, b.data.data_ptr(),
                                             b.rec.data_ptr(), s)
    else:
        rc = lib.cauchy_256_decode_batch_out_var(kmax, M, B, b.G, b.first.data_ptr(), b.total, b.blocks.data_ptr(),
                                                 b.rows.data_ptr(), b.out.data_ptr(), b.out_rows.data_ptr(),
                                                 b.cnt.data_ptr(), s)
    assert rc == 0


def leg_device(lib, ks, kmax, args, res, name):
    b = Batch(lib, ks, lambda bb: uniform_calls(lib, bb, "enc"))
    lib.cauchy_256_batch_reserve(kmax, M, B, b.G)
    r = res[name] = {"groups": b.G, "distinct_k": int(len(set(ks))), "blocks": b.total}
    for what in ("enc", "dec"):
        r["uniform_" + what + "_ms"] = [timed(lambda: uniform_calls(lib, b, what), args.iters, args.settle if i == 0 else 3)
                                        for i in range(3)]
    torch.cuda.synchronize()
    ref = (b.rec.clone(), b.out.clone(), b.out_rows.clone(), b.cnt.clone())
    assert int(ref[3].min()) == M and int(ref[3].max()) == M
    if not lib.has_var:
        return
    b.rec.zero_(), b.out.zero_(), b.out_rows.zero_(), b.cnt.zero_()
    for what in ("enc", "dec"):
        r["var_" + what + "_ms"] = [timed(lambda: var_call(lib, b, what, kmax), args.iters, 3) for _ in range(3)]
    torch.cuda.synchronize()
    assert lib.cauchy_256_batch_errors(torch.cuda.current_stream().cuda_stream) == 0
    same = all(torch.equal(x, y) for x, y in zip(ref, (b.rec, b.out, b.out_rows, b.cnt)))
    r["var_equals_uniform"] = bool(same)
    assert same, "var-k outputs differ from the uniform calls'"
    for what in ("enc", "dec"):
        r[what + "_var_over_uniform"] = float(np.median(r["var_" + what + "_ms"]) / np.median(r["uniform_" + what + "_ms"]))


TX = np.dtype([("k", "i4"), ("m", "i4"), ("packets", "u8"), ("lens", "u8"), ("out", "u8"), ("cap", "i4"),
               ("m_out", "i4"), ("stride", "i4")], align=True)
RX = np.dtype([("n_orig", "i4"), ("ids", "u8"), ("data", "u8"), ("lens", "u8"), ("n_rec", "i4"), ("rec", "u8"),
               ("rec_lens", "u8")], align=True)


def leg_host(lib, ks, args, res):
    ks = np.asarray(ks, np.int64)
    G, total, L = len(ks), int(ks.sum()), B - 2
    first = np.concatenate([[0], np.cumsum(ks)])
    pay = np.random.default_rng(1).integers(0, 256, size=total * L, dtype=np.uint8)
    ptrs = pay.ctypes.data + np.arange(total, dtype=np.uint64) * L
    lens = np.full(total, L, np.uint16)
    stride = 3 + B
    out = np.zeros(G * M * stride, np.uint8)
    tx = np.zeros(G, TX)
    tx["k"], tx["m"] = ks, M
    tx["packets"] = ptrs.ctypes.data + first[:-1].astype(np.uint64) * 8
    tx["lens"] = lens.ctypes.data + first[:-1].astype(np.uint64) * 2
    tx["out"] = out.ctypes.data + np.arange(G, dtype=np.uint64) * (M * stride)
    tx["cap"] = M * stride
    t = []
    for _ in range(args.host_reps + 1):
        t0 = time.perf_counter()
        assert lib.shorthair_encode_groups(tx.ctypes.data, G) == 0
        t.append(time.perf_counter() - t0)
    r = res["host"] = {"groups": G, "distinct_k": int(len(set(ks.tolist()))), "encode_groups_s": t[1:]}
    # receiver: every group lost its first M originals and got all M recovery packets
    ids = np.concatenate([np.arange(M, k, dtype=np.uint8) for k in ks])
    ofirst = np.concatenate([[0], np.cumsum(ks - M)])
    optrs = np.concatenate([ptrs[first[g] + M:first[g + 1]] for g in range(G)])
    olens = np.full(len(ids), L, np.uint16)
    rptrs = out.ctypes.data + np.arange(G * M, dtype=np.uint64) * stride
    rlens = np.full(G * M, stride, np.int32)
    rx = np.zeros(G, RX)
    rx["n_orig"], rx["n_rec"] = ks - M, M
    rx["ids"] = ids.ctypes.data + ofirst[:-1].astype(np.uint64)
    rx["data"] = optrs.ctypes.data + ofirst[:-1].astype(np.uint64) * 8
    rx["lens"] = olens.ctypes.data + ofirst[:-1].astype(np.uint64) * 2
    rx["rec"] = rptrs.ctypes.data + np.arange(G, dtype=np.uint64) * (M * 8)
    rx["rec_lens"] = rlens.ctypes.data + np.arange(G, dtype=np.uint64) * (M * 4)
    t = []
    for _ in range(args.host_reps + 1):
        t0 = time.perf_counter()
        assert lib.shorthair_recover_groups(rx.ctypes.data, G, None, None) == G
        t.append(time.perf_counter() - t0)
    r["recover_groups_s"] = t[1:]
    if hasattr(lib, "shorthair_groups_stats"):
        a, b = C.c_longlong(0), C.c_longlong(0)
        lib.shorthair_groups_stats(C.byref(a), C.byref(b))
        r["launches_total"], r["groups_total"] = a.value, b.value


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--lib", default=os.path.join(ROOT, "shorthair_amd", "libcauchy256.so"))
    p.add_argument("--out", required=True)
    p.add_argument("--groups", type=int, default=8192)
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--settle", type=int, default=40)
    p.add_argument("--host-reps", type=int, default=2)
    p.add_argument("--legs", default="headline,mixed,host")
    args = p.parse_args()
    lib = load(args.lib)
    res = {"lib": os.path.relpath(args.lib, ROOT), "has_var": lib.has_var, "m": M, "B": B, "iters": args.iters,
           "settle": args.settle, "device": torch.cuda.get_device_name(0)}
    legs = args.legs.split(",")
    mixed = np.sort(np.random.default_rng(7).integers(120, 201, size=args.groups))
    if "headline" in legs:
        leg_device(lib, [200] * args.groups, 200, args, res, "headline")
    if "mixed" in legs:
        leg_device(lib, mixed, 200, args, res, "mixed")
    if "host" in legs:
        leg_host(lib, np.random.default_rng(7).permutation(mixed), args, res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    sys.exit(main())
