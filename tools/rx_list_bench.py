"""Receive-listing measurement (DESIGN.md "Device-resident receive listing"): HIP-event times of
shorthair_rx_list_batch on the headline receive shape, beside shorthair_frame_batch and
cauchy_256_decode_batch_out_var on the lists it produced, in one process.

    python tools/rx_list_bench.py --out profiles/rx_list/<tag>.json

  k = 200, m = 32, B = 1400, 8192 groups, every group lost 32 originals: 168 original records
  "[id][id][1398 payload bytes]" and 32 recovery records "[200 + y][199][31][block]" per group, in a
  random arrival order, one record per ring slot of --slot bytes (so headers are --slot bytes apart).
  Each call is timed as `iters` back-to-back calls between two HIP events after settle calls; the three
  calls take turns, --repeats times, and the medians are reported; then single listing calls are timed
  right after a frame_batch pass over the ring, which leaves no header line in a cache. The lists are
  checked against the rule (restated here with numpy) before anything is timed.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
K, M, B, E = 200, 32, 1400, 32


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


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", required=True)
    p.add_argument("--groups", type=int, default=8192)
    p.add_argument("--slot", type=int, default=1408)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--settle", type=int, default=40)
    p.add_argument("--repeats", type=int, default=5)
    args = p.parse_args()
    import shorthair_amd as sh
    assert sh.cauchy_256_init() == 0
    G, slot = args.groups, args.slot
    assert slot >= 3 + B
    n = K  # records per group: K - E originals, E recovery
    P = G * n
    rng = np.random.default_rng(7)
    # arrival order per group: is_rec[g][i]; originals carry ids E..K-1 in a random order, recovery ids K..K+E-1
    is_rec = np.zeros((G, n), bool)
    is_rec[:, :E] = True
    is_rec = rng.permuted(is_rec, axis=1)
    ids = np.zeros((G, n), np.uint8)
    ids[~is_rec] = rng.permuted(np.tile(np.arange(E, K, dtype=np.uint8), (G, 1)), axis=1).reshape(-1)
    ids[is_rec] = rng.permuted(np.tile(np.arange(K, K + E, dtype=np.uint8), (G, 1)), axis=1).reshape(-1)
    hdr = np.zeros((P, 3), np.uint8)
    hdr[:, 0] = ids.reshape(-1)
    hdr[:, 1] = np.where(is_rec, K - 1, ids).reshape(-1)
    hdr[:, 2] = M - 1  # (in an original this is its first payload byte)
    pkt_first = (np.arange(G + 1, dtype=np.int64) * n).astype(np.int32)
    pkt_off = np.arange(P, dtype=np.int64) * slot
    pkt_len = np.where(is_rec, 3 + B, B).astype(np.int32).reshape(-1)
    ring_bytes = P * slot
    ring = torch.randint(0, 256, (P, slot), dtype=torch.uint8, device="cuda")
    ring[:, :3] = torch.from_numpy(hdr).cuda()
    d_first_in, d_off_in, d_len_in = (torch.from_numpy(a).cuda() for a in (pkt_first, pkt_off, pkt_len))
    cap = sh.rx_list_capacity(G, P, K)
    info = torch.empty((G, sh.RX_INFO_INTS), dtype=torch.int32, device="cuda")
    first = torch.empty(G + 1, dtype=torch.int32, device="cuda")
    slot_group = torch.empty(G, dtype=torch.int32, device="cuda")
    off = torch.empty(cap, dtype=torch.int64, device="cuda")
    length = torch.empty(cap, dtype=torch.int32, device="cuda")
    raw = torch.empty(cap, dtype=torch.uint8, device="cuda")
    rows = torch.empty(cap, dtype=torch.uint8, device="cuda")
    summary = torch.empty(8, dtype=torch.int32, device="cuda")
    scratch = torch.empty(sh.rx_list_scratch_bytes(G, P), dtype=torch.uint8, device="cuda")
    blocks = torch.empty((cap, B), dtype=torch.uint8, device="cuda")
    out = torch.empty((G, M, B), dtype=torch.uint8, device="cuda")
    out_rows = torch.empty((G, M), dtype=torch.uint8, device="cuda")
    count = torch.empty(G, dtype=torch.int32, device="cuda")

    def listing():
        assert sh.rx_list_batch(K, K, M, B, G, P, d_first_in, d_off_in, d_len_in, ring, ring_bytes, info, first,
                                slot_group, off, length, raw, rows, summary, scratch) == 0

    def frame():
        assert sh.frame_batch(B, cap, ring, ring_bytes, off, length, raw, blocks) == 0

    def decode():
        assert sh.decode_batch_out_var(K, M, B, G, first, cap, blocks, rows, out, out_rows, count) == 0

    # the lists against the rule: originals in arrival order, then the recovery records
    sh.batch_errors()
    listing()
    assert summary.cpu().tolist() == [G, G * K, 0, 0, 0, 0, 0, 0]
    order = np.argsort(is_rec, axis=1, kind="stable") + np.arange(G)[:, None] * n
    rec_sorted = is_rec.reshape(-1)[order.reshape(-1)]
    assert np.array_equal(off.cpu().numpy(), pkt_off[order.reshape(-1)] + 2 + rec_sorted)
    assert np.array_equal(length.cpu().numpy(), np.where(rec_sorted, B, B - 2))
    assert np.array_equal(raw.cpu().numpy(), rec_sorted.astype(np.uint8))
    assert np.array_equal(rows.cpu().numpy(), ids.reshape(-1)[order.reshape(-1)])
    assert np.array_equal(first.cpu().numpy(), np.arange(G + 1) * K)
    assert np.array_equal(slot_group.cpu().numpy(), np.arange(G))
    frame()
    decode()
    assert sh.batch_errors() == 0
    assert (count.cpu().numpy() == E).all()

    t = {"listing": [], "frame": [], "decode": []}
    for r in range(args.repeats):
        settle = args.settle if r == 0 else 3
        t["listing"].append(timed(listing, args.iters, settle))
        t["frame"].append(timed(frame, max(args.iters // 4, 2), min(settle, 5)))
        t["decode"].append(timed(decode, max(args.iters // 4, 2), min(settle, 5)))
    # back-to-back listing calls re-read the same header lines, which a last-level cache can hold; one call
    # right after a frame_batch pass over the whole ring (2.3 GB read, 2.3 GB written) finds them evicted
    t["listing_after_frame"] = []
    for _ in range(2 * args.repeats):
        frame()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        listing()
        e1.record()
        torch.cuda.synchronize()
        t["listing_after_frame"].append(e0.elapsed_time(e1))
    assert sh.batch_errors() == 0
    med = {name: float(np.median(v)) for name, v in t.items()}
    res = {"k": K, "m": M, "B": B, "e": E, "groups": G, "records": P, "records_per_group": n, "slot_bytes": slot,
           "iters": args.iters, "settle": args.settle, "repeats": args.repeats,
           "device": torch.cuda.get_device_name(0), "ms": t, "median_ms": med,
           "listing_over_decode": med["listing"] / med["decode"],
           "listing_after_frame_over_decode": med["listing_after_frame"] / med["decode"],
           "listing_over_frame_plus_decode": med["listing"] / (med["frame"] + med["decode"]),
           "records_per_us": P / med["listing"] / 1e3,
           "ring_bytes": ring_bytes,
           "ring_header_bytes_read": 3 * P,
           "ring_bytes_touched_as_64B_lines": 64 * P,
           "ring_bytes_touched_as_128B_lines": 128 * P,
           "input_array_bytes_read": 12 * P + 4 * (G + 1),
           "output_bytes_written": 14 * cap + 4 * (G * sh.RX_INFO_INTS + 2 * G + 1) + 32,
           "scratch_bytes": sh.rx_list_scratch_bytes(G, P),
           "decode_block_bytes_read": cap * B}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    sys.exit(main())
