"""Receive-window measurement (DESIGN.md "Open groups from one batch to the next"): HIP-event times of
shorthair_rx_window_batch on the headline receive shape, beside shorthair_rx_group_batch and
cauchy_256_decode_batch_out_var in the same process, and a device-to-device copy of the carried bytes.

    python tools/rx_window_bench.py --out profiles/rx_window/<tag>.json

  k = 200, m = 32, B = 1400, a window of 8192 slots, every group lost 32 originals; the traffic of
  tools/rx_group_bench.py (group g's recovery datagrams at random places among group g + 1's originals), one
  datagram per ring slot of --slot bytes, in two batches of --groups groups each. The cut between them falls
  among a run's datagrams, so the groups at the boundary straddle it. One allocation holds the two batches'
  ring regions and one hold region. Batch 1 goes through group -> window (a fresh receiver) -> list; batch 2
  through group -> window, which is the call that is timed, in two legs:

    steady   the listing's d_info over batch 1: the finished groups are dropped, their late datagrams
             ignored, the straddling groups carried
    worst    n_info = 0: nothing is finished, every record of batch 1 is carried

  Each call is timed as `iters` back-to-back calls between two HIP events after settle calls; the calls take
  turns, --repeats times; medians and ranges are reported. Every output array of both legs is compared with
  numpy, and every carried byte with its source on the device, before anything is timed.
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
W = 8192  # slots of the window


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


def traffic(rng, G):
    """(group, id, is_rec) per datagram of G groups in arrival order, as tools/rx_group_bench.py lays them."""
    is_rec = np.zeros((G + 1, K), bool)
    is_rec[:, :E] = True
    is_rec = rng.permuted(is_rec, axis=1)
    valid = np.ones((G + 1, K), bool)
    valid[0] = ~is_rec[0]
    valid[G] = is_rec[G]
    group = np.arange(G + 1)[:, None] - is_rec
    ids = np.zeros((G + 1, K), np.uint8)
    ids[~is_rec] = rng.permuted(np.tile(np.arange(E, K, dtype=np.uint8), (G + 1, 1)), axis=1).reshape(-1)
    ids[is_rec] = rng.permuted(np.tile(np.arange(K, K + E, dtype=np.uint8), (G + 1, 1)), axis=1).reshape(-1)
    return group[valid], ids[valid], is_rec[valid]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", required=True)
    p.add_argument("--groups", type=int, default=4096, help="groups per batch; two batches fill the window")
    p.add_argument("--slot", type=int, default=1408)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--settle", type=int, default=40)
    p.add_argument("--repeats", type=int, default=3)
    args = p.parse_args()
    import shorthair_amd as sh
    assert sh.cauchy_256_init() == 0
    Gh, slot = args.groups, args.slot
    assert slot >= 6 + B and slot % 16 == 0 and 2 * Gh <= W
    rng = np.random.default_rng(7)
    group, ids, is_rec = traffic(rng, 2 * Gh)
    N2 = len(group)
    cut = Gh * K - K // 3  # among the datagrams of one run of the interleaving: two groups straddle the cut
    n = [cut, N2 - cut]
    hdr = np.zeros((N2, 6), np.uint8)
    hdr[:, 0], hdr[:, 1] = np.arange(N2) & 255, (np.arange(N2) >> 8) & 255
    hdr[:, 2] = (FIRST_GROUP + group) & 127
    hdr[:, 3] = ids
    hdr[:, 4] = np.where(is_rec, K - 1, ids)
    hdr[:, 5] = M - 1
    dg_off = np.arange(N2, dtype=np.int64) * slot  # batch 1's region, then batch 2's, then the hold region
    dg_len = np.where(is_rec, 6 + B, 3 + B).astype(np.int32)
    hold_off, hold_bytes = N2 * slot, n[0] * slot
    ring_bytes = hold_off + hold_bytes
    ring = torch.empty(ring_bytes, dtype=torch.uint8, device="cuda")
    ring[:hold_off].view(N2, slot).copy_(torch.randint(0, 256, (N2, slot), dtype=torch.uint8, device="cuda"))
    ring[:hold_off].view(N2, slot)[:, :6] = torch.from_numpy(hdr).cuda()
    ring[hold_off:] = 0
    d_off, d_len = torch.from_numpy(dg_off).cuda(), torch.from_numpy(dg_len).cuda()
    i32 = lambda k: torch.empty(k, dtype=torch.int32, device="cuda")  # noqa: E731
    u8 = lambda k: torch.empty(k, dtype=torch.uint8, device="cuda")  # noqa: E731
    state = [torch.tensor([FIRST_GROUP], dtype=torch.int32, device="cuda"), i32(1), i32(1)]
    grp = [dict(dg_class=i32(k), dg_slot=i32(k), pkt_first=i32(W + 1), pkt_off=torch.empty(k, dtype=torch.int64, device="cuda"),
                pkt_len=i32(k), pkt_dg=i32(k), slot_group=i32(W), other=i32(k), summary=i32(8),
                scratch=u8(sh.rx_group_scratch_bytes(k, W))) for k in n]
    cap = N2
    win = [sh.RxWindow(W, cap), sh.RxWindow(W, cap)]
    wsum, wscratch = torch.zeros(8, dtype=torch.int64, device="cuda"), u8(sh.rx_window_scratch_bytes(W, cap))
    lcap = sh.rx_list_capacity(W, cap, K)
    info, first, slot_group, length, lsum = i32(W * sh.RX_INFO_INTS).view(W, -1), i32(W + 1), i32(W), i32(lcap), i32(8)
    off = torch.empty(lcap, dtype=torch.int64, device="cuda")
    raw, rows, lscratch = u8(lcap), u8(lcap), u8(sh.rx_list_scratch_bytes(W, cap))
    blocks = torch.empty((lcap, B), dtype=torch.uint8, device="cuda")
    out, out_rows, count = u8(W * M * B).view(W, M, B), u8(W * M).view(W, M), i32(W)

    def grouping(j, back):
        a, g = (0, n[0]) if j == 0 else (n[0], N2), grp[j]
        assert sh.rx_group_batch(n[j], W, back, d_off[a[0]:a[1]], d_len[a[0]:a[1]], ring, ring_bytes, state[j], state[j + 1],
                                 g["dg_class"], g["dg_slot"], g["pkt_first"], g["pkt_off"], g["pkt_len"], g["pkt_dg"],
                                 g["slot_group"], g["other"], g["summary"], g["scratch"]) == 0

    def window(j, prev, infos):
        g = grp[j]
        assert sh.rx_window_batch(W, prev, infos, n[j], g["pkt_first"], g["pkt_off"], g["pkt_len"], g["pkt_dg"],
                                  g["slot_group"], ring, ring_bytes, hold_off, hold_bytes, win[j], wsum, wscratch) == 0

    def listing(j):
        assert sh.rx_list_batch(K, K, M, B, W, cap, win[j].first, win[j].off, win[j].len, ring, ring_bytes, info, first,
                                slot_group, off, length, raw, rows, lsum, lscratch) == 0

    def decode():
        assert sh.decode_batch_out_var(K, M, B, W, first, lcap, blocks, rows, out, out_rows, count) == 0

    # batch 1: a fresh receiver
    sh.batch_errors()
    grouping(0, 0)
    window(0, None, [])
    listing(0)
    info1 = info.clone()
    in1 = np.arange(N2) < cut
    done1 = np.bincount(group[in1], minlength=W)[:W] == K  # the groups batch 1 holds completely
    assert np.array_equal(info1.cpu().numpy()[:, 0] == 1, done1) and abs(int(done1.sum()) - Gh) <= 3
    straddling = np.intersect1d(group[in1], group[~in1]).tolist()
    assert len(straddling) >= 2
    back2 = int(state[1].cpu()[0]) - FIRST_GROUP  # batch 2's window starts where batch 1's does
    assert 0 < back2 < W
    grouping(1, back2)
    assert grp[1]["summary"].cpu().tolist()[:2] == [n[1], 0]

    def expected(steady):
        """The next window by numpy: per slot the carried records in arrival order, then the new ones."""
        keep1 = in1 & ~done1[group] if steady else in1
        keep2 = ~in1 & ~done1[group] if steady else ~in1
        idx = np.flatnonzero(keep1 | keep2)
        idx = idx[np.argsort(group[idx], kind="stable")]  # (arrival order puts batch 1 in front of batch 2)
        carried = idx < cut
        ln = dg_len[idx] - 3
        place = np.concatenate([[0], np.cumsum(np.where(carried, (ln + 15) // 16 * 16, 0))])
        eoff = np.where(carried, hold_off + place[:-1], dg_off[idx] + 3)
        edg = np.where(carried, -1, idx - cut)
        efirst = np.concatenate([[0], np.cumsum(np.bincount(group[idx], minlength=W)[:W])])
        esum = [len(idx), int(carried.sum()), int(place[-1]), int(done1.sum()) if steady else 0, 0,
                int((~in1 & done1[group]).sum()) if steady else 0, 0, 0]
        return idx, carried, eoff, ln, edg, efirst, (done1 if steady else np.zeros(W, bool)).astype(np.uint8), esum

    def check(steady):
        idx, carried, eoff, ln, edg, efirst, edone, esum = expected(steady)
        total = len(idx)
        w = win[1]
        assert wsum.cpu().tolist() == esum, (wsum.cpu().tolist(), esum)
        assert int(w.base.cpu()[0]) == FIRST_GROUP and np.array_equal(w.first.cpu().numpy(), efirst)
        assert np.array_equal(w.done.cpu().numpy(), edone)
        assert np.array_equal(w.off.cpu().numpy()[:total], eoff) and not w.off.cpu().numpy()[total:].any()
        assert np.array_equal(w.len.cpu().numpy()[:total], ln) and not w.len.cpu().numpy()[total:].any()
        assert np.array_equal(w.dg.cpu().numpy()[:total], edg) and (w.dg.cpu().numpy()[total:] == -1).all()
        # every carried byte against its source, on the device
        src = torch.from_numpy(idx[carried]).cuda()
        dst = torch.from_numpy((eoff[carried] - hold_off) // slot).cuda()
        assert np.array_equal((eoff[carried] - hold_off) % slot, np.zeros(carried.sum(), np.int64))
        held = ring[hold_off:].view(n[0], slot)
        for a in range(0, len(src), 65536):
            got = held[dst[a:a + 65536]]
            want = ring[:hold_off].view(N2, slot)[src[a:a + 65536]]
            lens = torch.from_numpy(ln[carried][a:a + 65536]).cuda()[:, None]
            col = torch.arange(slot - 3, device="cuda")[None, :]
            assert bool(((got[:, :slot - 3] == want[:, 3:]) | (col >= lens)).all())
        return esum

    ring[hold_off:] = 0
    window(1, win[0], [info1])
    steady = check(True)
    listing(1)
    assert sh.frame_batch(B, lcap, ring, ring_bytes, off, length, raw, blocks) == 0
    decode()
    listed = int(lsum.cpu()[0])
    assert listed >= Gh - 2 and sh.batch_errors() == W - listed  # (the empty tail slots of the decode's upper bound)
    ring[hold_off:] = 0
    window(1, win[0], [])
    worst = check(False)
    assert worst[1] == n[0]
    carried_bytes = {"steady": int((dg_len[np.flatnonzero(in1 & ~done1[group])] - 3).sum()), "worst": int((dg_len[in1] - 3).sum())}
    a_copy, b_copy = u8(carried_bytes["worst"]), u8(carried_bytes["worst"])
    a_small, b_small = u8(carried_bytes["steady"]), u8(carried_bytes["steady"])

    legs = {"window_steady": lambda: window(1, win[0], [info1]), "window_worst": lambda: window(1, win[0], []),
            "grouping": lambda: grouping(1, back2), "decode": decode,
            "copy_worst_bytes": lambda: b_copy.copy_(a_copy), "copy_steady_bytes": lambda: b_small.copy_(a_small)}
    t = {name: [] for name in legs}
    for r in range(args.repeats):
        for name, fn in legs.items():  # every leg settles with the full count before each of its timings
            t[name].append(timed(fn, max(args.iters // 4, 2) if name == "decode" else args.iters, args.settle))
    window(1, win[0], [info1])
    check(True)  # the outputs after the timed runs are still the rule's
    med = {name: float(np.median(v)) for name, v in t.items()}
    res = {"k": K, "m": M, "B": B, "e": E, "window_slots": W, "groups_per_batch": Gh, "datagrams": n, "slot_bytes": slot,
           "cut_at_datagram": cut, "groups_straddling_the_cut": straddling,
           "iters": args.iters, "settle": args.settle, "repeats": args.repeats,
           "device": torch.cuda.get_device_name(0), "ms": t, "median_ms": med,
           "range_ms": {name: [float(min(v)), float(max(v))] for name, v in t.items()},
           "summary": {"steady": steady, "worst": worst}, "carried_bytes": carried_bytes,
           "copy_over_call_worst": med["copy_worst_bytes"] / med["window_worst"],
           "copy_over_call_steady": med["copy_steady_bytes"] / med["window_steady"],
           "window_steady_over_grouping": med["window_steady"] / med["grouping"],
           "window_steady_over_decode": med["window_steady"] / med["decode"],
           "worst_GBps_read_plus_written": 2 * carried_bytes["worst"] / med["window_worst"] / 1e6,
           "scratch_bytes": sh.rx_window_scratch_bytes(W, cap)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    sys.exit(main())
