"""Send-side datagram measurement (DESIGN.md "Datagrams as they leave"): HIP-event times of
shorthair_tx_datagram_batch on the headline send shape, beside a device-to-device copy of the same number of
bytes and the encode of the same batch, in one process.

    python tools/tx_bench.py --out profiles/tx/<tag>.json

  k = 200, m = 32, B = 1400, 8192 groups: 200 originals "[seq u16][g & 0x7f][id][id][payload]" and 32 recovery
  datagrams "[seq u16][g & 0x7f][200 + y][199][31][block]" per group, interleaved as a sender interleaves them:
  group g's recovery datagrams fall, at random places, among group g + 1's originals. Two legs: every payload
  1398 bytes ("full"), and payloads of 8..1350 bytes with one of 1398 per group ("short"). Payload j lies at
  byte 1400 j + 2 of a buffer of random bytes -- where a framed block would hold it -- and the encode runs on
  that buffer as its blocks. Each leg is timed with align = 16 and align = 1. Each call is timed as `iters`
  back-to-back calls between two HIP events after settle calls, the calls taking turns, --repeats times;
  medians and ranges are reported. Before anything is timed the lengths, classes and offsets of every
  datagram and the bytes of a sample of them are checked against numpy.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
K, M, B = 200, 32, 1400
U0, SEQ0 = 1000, 50000


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


def schedule(rng, G):
    """Run j = group j's originals in order with group j - 1's recovery datagrams at random places."""
    is_rec = np.zeros((G + 1, K + M), bool)
    is_rec[:, :M] = True
    is_rec = rng.permuted(is_rec, axis=1)
    x = np.cumsum(~is_rec, axis=1) - 1
    y = np.cumsum(is_rec, axis=1) - 1
    j = np.arange(G + 1, dtype=np.int64)[:, None]
    e = np.where(is_rec, ((j - 1) << 9) | 256 | y, (j << 9) | x)
    valid = np.ones_like(is_rec)
    valid[0] = ~is_rec[0]   # (no group in front of the first)
    valid[G] = is_rec[G]    # (and no originals behind the last)
    return e[valid].astype(np.int32)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", required=True)
    p.add_argument("--groups", type=int, default=8192)
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--settle", type=int, default=40)
    p.add_argument("--repeats", type=int, default=3)
    args = p.parse_args()
    import shorthair_amd as sh
    assert sh.cauchy_256_init() == 0
    G = args.groups
    N, total = G * (K + M), G * K
    rng = np.random.default_rng(11)
    sched = schedule(rng, G)
    assert len(sched) == N
    data = torch.randint(0, 256, (total * B,), dtype=torch.uint8, device="cuda")  # blocks [G][K][B]; payload j at 1400 j + 2
    rec = torch.empty(G * M * B, dtype=torch.uint8, device="cuda")
    assert sh.encode_batch(K, M, B, G, data, rec) == 0
    off = np.arange(total, dtype=np.int64) * B + 2
    lens = {"full": np.full(total, B - 2, np.int32)}
    short = rng.integers(8, 1351, size=total).astype(np.int32)
    short[np.arange(G) * K + rng.integers(0, K, size=G)] = B - 2
    lens["short"] = short
    d_sched, d_first, d_off = (torch.from_numpy(a).cuda() for a in (sched, (np.arange(G + 1) * K).astype(np.int32), off))
    state = torch.tensor([SEQ0, U0], dtype=torch.int32, device="cuda")
    state_out = torch.empty(2, dtype=torch.int32, device="cuda")
    dg_off = torch.empty(N + 1, dtype=torch.int64, device="cuda")
    dg_len, dg_class, summary = (torch.empty(n, dtype=torch.int32, device="cuda") for n in (N, N, 8))
    scratch = torch.empty(sh.tx_datagram_scratch_bytes(N), dtype=torch.uint8, device="cuda")
    ring_bytes = sh.tx_datagram_capacity(N, 6 + B, 16)
    ring = torch.empty(ring_bytes, dtype=torch.uint8, device="cuda")
    src = torch.empty(ring_bytes, dtype=torch.uint8, device="cuda")
    g_of, x_of = sched.astype(np.int64) >> 9, sched & 511
    is_rec = x_of >= 256

    def encode():
        assert sh.encode_batch(K, M, B, G, data, rec) == 0

    res = {"k": K, "m": M, "B": B, "groups": G, "datagrams": N, "iters": args.iters, "settle": args.settle,
           "repeats": args.repeats, "device": torch.cuda.get_device_name(0),
           "interleaving": "group g's recovery datagrams at random places among group g + 1's originals", "legs": {}}
    sh.batch_errors()
    for leg, ln in lens.items():
        d_len = torch.from_numpy(ln).cuda()
        want_len = np.where(is_rec, 6 + B, 5 + ln[np.minimum(g_of * K + (x_of & 255), total - 1)]).astype(np.int64)
        written = int(want_len.sum())

        def tx(align):
            assert sh.tx_datagram_batch(N, G, M, B, d_sched, d_first, total, data, data.numel(), d_off, d_len, rec, rec.numel(),
                                        None, 0, None, None, G, state, state_out, align, ring, ring_bytes, dg_off, dg_len,
                                        dg_class, summary, scratch) == 0

        def copy():
            ring[:written].copy_(src[:written])

        # the outputs against numpy: every length, class and offset, and the bytes of a sample
        for align in (16, 1):
            ring.zero_()
            tx(align)
            step = (want_len + align - 1) // align * align
            want_off = np.concatenate([[0], np.cumsum(step)])
            assert np.array_equal(dg_off.cpu().numpy(), want_off) and np.array_equal(dg_len.cpu().numpy(), want_len)
            assert np.array_equal(dg_class.cpu().numpy(), is_rec.astype(np.int32))
            assert summary.cpu().tolist() == [N, total, G * M, 0, 0, 0, 0, 0] and state_out.cpu().tolist() == [SEQ0 + N, U0 + G]
            data_h, rec_h = data[:64 * K * B].cpu().numpy(), rec[:64 * M * B].cpu().numpy()
            for i in list(range(300)) + [int(v) for v in rng.integers(0, 60 * (K + M), size=300)]:
                g, x, seq = int(g_of[i]), int(x_of[i]), (SEQ0 + i) & 0xffff
                if x < 256:
                    j = g * K + x
                    want = bytes([seq & 255, seq >> 8, (U0 + g) & 127, x, x]) + data_h[off[j]:off[j] + ln[j]].tobytes()
                else:
                    at = (g * M + x - 256) * B
                    want = bytes([seq & 255, seq >> 8, (U0 + g) & 127, K + x - 256, K - 1, M - 1]) + rec_h[at:at + B].tobytes()
                o = int(want_off[i])
                assert ring[o:o + len(want)].cpu().numpy().tobytes() == want, (leg, align, i)
        t = {"tx_align16": [], "tx_align1": [], "copy": [], "encode": []}
        for r in range(args.repeats):
            settle = args.settle if r == 0 else 3
            t["tx_align16"].append(timed(lambda: tx(16), args.iters, settle))
            t["tx_align1"].append(timed(lambda: tx(1), args.iters, settle))
            t["copy"].append(timed(copy, args.iters, settle))
            t["encode"].append(timed(encode, max(args.iters // 2, 2), min(settle, 5)))
        med = {name: float(np.median(v)) for name, v in t.items()}
        res["legs"][leg] = {
            "payload_bytes": "1398" if leg == "full" else "8..1350, one of 1398 per group",
            "bytes_written": written, "ring_bytes_align16": int(((want_len + 15) // 16 * 16).sum()),
            "bytes_read": written - 5 * total - 6 * G * M, "ms": t, "median_ms": med,
            "range_ms": {name: [float(min(v)), float(max(v))] for name, v in t.items()},
            "tx_gb_written_per_s": written / med["tx_align16"] / 1e6,
            "copy_gb_per_s": written / med["copy"] / 1e6,
            "copy_over_tx": med["copy"] / med["tx_align16"],
            "tx_over_encode": med["tx_align16"] / med["encode"],
            "align1_over_align16": med["tx_align1"] / med["tx_align16"]}
    assert sh.batch_errors() == 0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    sys.exit(main())
