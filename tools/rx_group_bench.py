"""Receive-grouping measurement (DESIGN.md "Datagrams as they arrive"): HIP-event times of
shorthair_rx_group_batch on the headline receive shape, beside shorthair_rx_list_batch and
cauchy_256_decode_batch_out_var on its output, in one process.

    python tools/rx_group_bench.py --out profiles/rx_group/<tag>.json

  k = 200, m = 32, B = 1400, 8192 groups, every group lost 32 originals: 168 data datagrams
  "[seq u16][g & 0x7f][id][id][1398 payload bytes]" and 32 recovery datagrams
  "[seq u16][g & 0x7f][200 + y][199][31][block]" per group, one datagram per ring slot of --slot bytes. The
  groups are interleaved as a sender interleaves them: group g's recovery datagrams fall, at random places,
  among group g + 1's originals. The host passes only the (offset, length) pairs in arrival order and the
  state. Each call is timed as `iters` back-to-back calls between two HIP events after settle calls; the
  three calls take turns, --repeats times; medians and ranges are reported. The CSR is checked against a
  stable sort by group (numpy) and the decode's counts against the loss before anything is timed.
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
FIRST_GROUP = 1000


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
    assert slot >= 6 + B
    n_orig = K - E
    N = G * K
    rng = np.random.default_rng(7)
    # arrival order: run j = group j's originals with group j - 1's recovery datagrams among them
    is_rec = np.zeros((G + 1, K), bool)
    is_rec[:, :E] = True
    is_rec = rng.permuted(is_rec, axis=1)
    valid = np.ones((G + 1, K), bool)
    valid[0] = ~is_rec[0]   # (no group in front of the first)
    valid[G] = is_rec[G]    # (and no originals behind the last)
    group = np.arange(G + 1)[:, None] - is_rec
    ids = np.zeros((G + 1, K), np.uint8)
    ids[~is_rec] = rng.permuted(np.tile(np.arange(E, K, dtype=np.uint8), (G + 1, 1)), axis=1).reshape(-1)
    ids[is_rec] = rng.permuted(np.tile(np.arange(K, K + E, dtype=np.uint8), (G + 1, 1)), axis=1).reshape(-1)
    is_rec, group, ids = is_rec[valid], group[valid], ids[valid]
    assert len(group) == N
    hdr = np.zeros((N, 6), np.uint8)
    hdr[:, 0], hdr[:, 1] = np.arange(N) & 255, (np.arange(N) >> 8) & 255
    hdr[:, 2] = (FIRST_GROUP + group) & 127
    hdr[:, 3] = ids
    hdr[:, 4] = np.where(is_rec, K - 1, ids)
    hdr[:, 5] = M - 1  # (in an original this is its first payload byte)
    dg_off = np.arange(N, dtype=np.int64) * slot
    dg_len = np.where(is_rec, 6 + B, 3 + B).astype(np.int32)
    ring_bytes = N * slot
    ring = torch.randint(0, 256, (N, slot), dtype=torch.uint8, device="cuda")
    ring[:, :6] = torch.from_numpy(hdr).cuda()
    d_dg_off, d_dg_len = torch.from_numpy(dg_off).cuda(), torch.from_numpy(dg_len).cuda()
    state_in = torch.tensor([FIRST_GROUP], dtype=torch.int32, device="cuda")
    i32 = lambda k: torch.empty(k, dtype=torch.int32, device="cuda")  # noqa: E731
    u8 = lambda k: torch.empty(k, dtype=torch.uint8, device="cuda")  # noqa: E731
    state_out, dg_class, dg_slot, pkt_first, pkt_len, pkt_dg = i32(1), i32(N), i32(N), i32(G + 1), i32(N), i32(N)
    pkt_off = torch.empty(N, dtype=torch.int64, device="cuda")
    gslot_group, other, gsummary = i32(G), i32(N), i32(8)
    gscratch = u8(sh.rx_group_scratch_bytes(N, G))
    cap = sh.rx_list_capacity(G, N, K)
    info, first, slot_group, length, summary = i32(G * sh.RX_INFO_INTS).view(G, -1), i32(G + 1), i32(G), i32(cap), i32(8)
    off = torch.empty(cap, dtype=torch.int64, device="cuda")
    raw, rows, scratch = u8(cap), u8(cap), u8(sh.rx_list_scratch_bytes(G, N))
    blocks = torch.empty((cap, B), dtype=torch.uint8, device="cuda")
    out, out_rows, count = u8(G * M * B).view(G, M, B), u8(G * M).view(G, M), i32(G)

    def grouping():
        assert sh.rx_group_batch(N, G, 0, d_dg_off, d_dg_len, ring, ring_bytes, state_in, state_out, dg_class, dg_slot,
                                 pkt_first, pkt_off, pkt_len, pkt_dg, gslot_group, other, gsummary, gscratch) == 0

    def listing():
        assert sh.rx_list_batch(K, K, M, B, G, N, pkt_first, pkt_off, pkt_len, ring, ring_bytes, info, first,
                                slot_group, off, length, raw, rows, summary, scratch) == 0

    def decode():
        assert sh.decode_batch_out_var(K, M, B, G, first, cap, blocks, rows, out, out_rows, count) == 0

    # the CSR against a stable sort by group; the chain against the loss
    sh.batch_errors()
    grouping()
    order = np.argsort(group, kind="stable")
    assert gsummary.cpu().tolist() == [N, 0, 0, G, 0, 0, 0, 0]
    assert int(state_out.cpu()[0]) == FIRST_GROUP + G - 1
    assert np.array_equal(pkt_dg.cpu().numpy(), order)
    assert np.array_equal(pkt_off.cpu().numpy(), dg_off[order] + 3)
    assert np.array_equal(pkt_len.cpu().numpy(), dg_len[order] - 3)
    assert np.array_equal(pkt_first.cpu().numpy(), np.arange(G + 1) * K)
    assert np.array_equal(dg_slot.cpu().numpy(), group) and not dg_class.cpu().numpy().any()
    assert np.array_equal(gslot_group.cpu().numpy(), FIRST_GROUP + np.arange(G)) and (other.cpu().numpy() == -1).all()
    listing()
    assert summary.cpu().tolist() == [G, G * K, 0, 0, 0, 0, 0, 0]
    assert sh.frame_batch(B, cap, ring, ring_bytes, off, length, raw, blocks) == 0
    decode()
    assert sh.batch_errors() == 0
    assert (count.cpu().numpy() == E).all()

    t = {"grouping": [], "listing": [], "decode": []}
    for r in range(args.repeats):
        settle = args.settle if r == 0 else 3
        t["grouping"].append(timed(grouping, args.iters, settle))
        t["listing"].append(timed(listing, args.iters, settle))
        t["decode"].append(timed(decode, max(args.iters // 4, 2), min(settle, 5)))
    assert sh.batch_errors() == 0
    med = {name: float(np.median(v)) for name, v in t.items()}
    res = {"k": K, "m": M, "B": B, "e": E, "groups": G, "datagrams": N, "datagrams_per_group": K, "slot_bytes": slot,
           "interleaving": "group g's recovery datagrams at random places among group g + 1's originals",
           "iters": args.iters, "settle": args.settle, "repeats": args.repeats,
           "device": torch.cuda.get_device_name(0), "ms": t, "median_ms": med,
           "range_ms": {name: [float(min(v)), float(max(v))] for name, v in t.items()},
           "grouping_over_decode": med["grouping"] / med["decode"],
           "grouping_over_listing": med["grouping"] / med["listing"],
           "datagrams_per_us": N / med["grouping"] / 1e3,
           "ring_bytes": ring_bytes,
           "ring_header_bytes_read": N,
           "input_array_bytes_read": 12 * N + 4,
           "output_bytes_written": 28 * N + 4 * (2 * G + 1) + 36,
           "scratch_bytes": sh.rx_group_scratch_bytes(N, G)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    sys.exit(main())
