"""Recovered packet groups unframed on the GPU (include/shorthair_groups.h: shorthair_groups_set_delivery(1)).

Delivery 1 runs shorthair_unframe_batch on every m >= 2 chunk and brings back only the packed payloads,
in two phases; callbacks, return values and launch counts must equal delivery 0's on both framing
routes and the oracle's (oracle/packets.py on the CPU oracle), and shorthair_groups_traffic must show
the D2H bytes the layout allows and no more.
"""
import ctypes
import random

import numpy as np
import pytest

from oracle import packets as opk
from oracle import pyoracle as po


# ---------------------------------------------------------------- CPU

def test_set_delivery_returns_previous_and_rejects_others():
    from shorthair_amd import groups as sg
    import shorthair_amd as sh
    f = sh.lib.shorthair_groups_set_delivery
    try:
        assert f(0) == 0          # the default
        assert f(1) == 0 and f(1) == 1 and f(0) == 1
        for bad in (2, -1, 3, 1 << 20):
            assert f(bad) == -1
            assert f(0) == 0      # a rejected argument changes nothing
        assert sg.set_delivery(1) == 0 and sg.set_delivery(0) == 1
        with pytest.raises(ValueError):
            sg.set_delivery(2)
        assert sh.lib.shorthair_groups_set_framing(0) == 0  # the two switches are independent
    finally:
        f(0)


# ---------------------------------------------------------------- workload (that of test_groups_frame.py)

SHORT_K, SHORT_M, SHORT_LONG = 30, 4, 1350  # short-payload groups: B = roundup8(2 + 1350) = 1352


def _payload(nprng, n):
    return nprng.integers(0, 256, size=int(n), dtype=np.uint8).tobytes()


def _workload():
    """About 40 groups: k = 1, a uniform bucket, a mixed-k bucket, m = 1, full-size payloads, zero-length
    payloads, and short-payload groups. Every m >= 2 group has k >= m, so whatever bucket a group lands
    in, its emax = min(k or kmax, m) is m. Returns (groups, indices of the short ones)."""
    nprng = np.random.default_rng(2025)
    groups = []
    groups.append((3, [_payload(nprng, 40)]))                      # k = 1
    groups.append((1, [b""]))                                      # k = 1, empty payload
    for _ in range(5):                                             # uniform bucket: k = 10, m = 4, B = 256
        lens = [int(v) for v in nprng.integers(1, 255, size=10)]
        lens[3] = 254
        groups.append((4, [_payload(nprng, n) for n in lens]))
    for i in range(16):                                            # mixed-k bucket (m = 4, B = 256)
        k = 17 + (i * 5) % 12
        lens = [int(v) for v in nprng.integers(0, 255, size=k)]
        lens[0], lens[1] = 254, 0                                  # a zero-length payload in each
        groups.append((4, [_payload(nprng, n) for n in lens]))
    for k in (5, 5, 9):                                            # m = 1 (a uniform pair and a single)
        lens = [int(v) for v in nprng.integers(0, 100, size=k)]
        lens[-1] = 100
        groups.append((1, [_payload(nprng, n) for n in lens]))
    groups.append((6, [_payload(nprng, 510) for _ in range(12)]))  # every payload full size: B = 512
    groups.append((2, [b"", b""]))                                 # nothing but empty payloads: B = 8
    short = list(range(len(groups), len(groups) + 10))
    for _ in range(10):                                            # short payloads, one long one: B = 1352
        lens = [int(v) for v in nprng.integers(0, 65, size=SHORT_K)]
        lens[int(nprng.integers(0, SHORT_K))] = SHORT_LONG
        groups.append((SHORT_M, [_payload(nprng, n) for n in lens]))
    groups += [(4, [_payload(nprng, n) for n in [254] + [7] * 20])]  # one more k for the mixed bucket
    order = list(range(len(groups)))
    random.Random(6).shuffle(order)
    shuffled = [groups[i] for i in order]
    return shuffled, sorted(order.index(i) for i in short)


def _receive(groups, recs, seed):
    """One receive pattern per group -- a random number e of losses: (originals, recovery packets) in
    arrival order."""
    rng = random.Random(seed)
    rx = []
    for (m, pk), rec in zip(groups, recs):
        k = len(pk)
        if k == 1:
            rx.append(([], rec[:1]) if rng.random() < 0.7 else ([(0, pk[0])], rec[:1]))
            continue
        e = rng.randint(1, min(k, len(rec)))
        lost = set(rng.sample(range(k), e))
        orig = [(i, pk[i]) for i in range(k) if i not in lost]
        rng.shuffle(orig)
        got = rng.sample(rec, rng.randint(e, len(rec)))
        rx.append((orig, got))
    return rx


def _oracle_deliveries(ora, rx):
    n, out = 0, []
    for g, (orig, rec) in enumerate(rx):
        got = opk.rx_group(ora, orig, rec)
        if got is not None:
            n += 1
            out += [(g, pid, p) for pid, p in got]
    return n, out


def _d2h_bound(groups, rx, want, launches):
    """What a delivery-1 call may copy device to host, from the layout: the delivered payload bytes of
    the m >= 2 buckets, 5 bytes per slot (len 4, row 1; slots = sum of gn * emax, emax = m here), 64
    bytes per launch (the 8-byte total), and the m = 1 buckets' blocks as delivery 0 counts them."""
    decoded = {g for g, _, _ in want}
    payload = sum(len(p) for g, _, p in want if len(groups[g][1]) >= 2 and groups[g][0] >= 2)
    slots = sum(m for g, (m, pk) in enumerate(groups) if g in decoded and len(pk) >= 2 and m >= 2)
    m1 = sum(opk.roundup8(2 + max(len(p) for p in pk)) for g, (m, pk) in enumerate(groups)
             if g in decoded and len(pk) >= 2 and m == 1)
    return payload + 5 * slots + 64 * launches + m1, slots


def test_workload_covers_the_cases():
    groups, short = _workload()
    assert 38 <= len(groups) <= 45 and len(short) == 10
    assert [len(pk) for _, pk in groups].count(1) == 2
    assert sum(1 for m, pk in groups if m == 1 and len(pk) > 1) == 3
    assert any(len(p) == 0 for _, pk in groups for p in pk)
    assert all(len(pk) >= m for m, pk in groups if m >= 2 and len(pk) >= 2)  # emax = m in every bucket
    for m, pk in (groups[i] for i in short):
        assert len(pk) == SHORT_K and m == SHORT_M and opk.roundup8(2 + max(len(p) for p in pk)) == 1352
        assert sorted(len(p) for p in pk)[-2] <= 64


# ---------------------------------------------------------------- GPU

def _recover(sh, sg, rx):
    l0, g0 = sh.groups_stats()
    t0 = sg.traffic()
    n, delivered = sg.recover_groups(rx)
    l1, g1 = sh.groups_stats()
    t1 = sg.traffic()
    return n, delivered, (l1 - l0, g1 - g0), t1[1] - t0[1]


@pytest.mark.gpu
def test_device_delivery_matches_host_delivery_and_oracle():
    import shorthair_amd as sh
    from shorthair_amd import groups as sg
    ora = po.oracle()
    groups, short = _workload()
    expect = [opk.tx_group(ora, m, pk) for m, pk in groups]
    rx = _receive(groups, expect, seed=14)
    want_n, want = _oracle_deliveries(ora, rx)
    assert sg.set_framing(0) == 0 and sg.set_delivery(0) == 0
    try:
        res = {}
        for framing in (0, 1):
            for delivery in (0, 1):
                sg.set_framing(framing)
                sg.set_delivery(delivery)
                res[framing, delivery] = _recover(sh, sg, rx)
        base = res[0, 0]
        for key, (n, delivered, stats, d2h) in res.items():
            assert n == want_n == base[0], key
            assert delivered == base[1], key             # the same callbacks in the same order
            assert stats == base[2], key                 # the same launches over the same groups
            by_group = {}                                # and per group the oracle's: ids, payloads, order
            for g, pid, p in delivered:
                by_group.setdefault(g, []).append((g, pid, p))
            assert sorted(by_group) == sorted({g for g, _, _ in want}), key
            assert [d for g in sorted(by_group) for d in by_group[g]] == want, key
        assert base[2][1] == sum(1 for (orig, rec), (_, pk) in zip(rx, groups) if len(pk) >= 2)

        # D2H accounting of a delivery-1 call, whole workload
        for framing in (0, 1):
            bound, slots = _d2h_bound(groups, rx, want, res[framing, 1][2][0])
            print("framing", framing, "d2h delivery 0 / 1 / bound:", res[framing, 0][3], res[framing, 1][3], bound)
            assert slots > 0 and 0 < res[framing, 1][3] <= bound

        # and on the short-payload groups alone: within the bound, strictly below delivery 0
        sel = [groups[i] for i in short]
        sel_rx = [rx[i] for i in short]
        sel_n, sel_want = _oracle_deliveries(ora, sel_rx)
        for framing in (0, 1):
            sg.set_framing(framing)
            d2h = {}
            for delivery in (0, 1):
                sg.set_delivery(delivery)
                n, delivered, stats, d2h[delivery] = _recover(sh, sg, sel_rx)
                assert n == sel_n == len(sel) and delivered == sel_want
            bound, slots = _d2h_bound(sel, sel_rx, sel_want, stats[0])
            print("short groups, framing", framing, "d2h delivery 0 / 1 / bound:", d2h[0], d2h[1], bound)
            assert slots == len(sel) * SHORT_M
            assert d2h[0] >= slots * 1352
            assert 0 < d2h[1] <= bound and d2h[1] < d2h[0]
    finally:
        sg.set_delivery(0)
        sg.set_framing(0)


def _rx_array(sg, groups):
    """The ctypes ShorthairRxGroup array shorthair_amd.groups.recover_groups builds."""
    _c = ctypes
    keep, rx = [], (sg.RxGroup * max(1, len(groups)))()
    for i, (orig, rec) in enumerate(groups):
        ids = (_c.c_ubyte * max(1, len(orig)))(*[o[0] for o in orig])
        obufs = [_c.create_string_buffer(bytes(o[1]), max(1, len(o[1]))) for o in orig]
        oarr = (_c.c_void_p * max(1, len(orig)))(*[_c.addressof(b) for b in obufs])
        olens = (_c.c_ushort * max(1, len(orig)))(*[len(o[1]) for o in orig])
        rbufs = [_c.create_string_buffer(bytes(r), max(1, len(r))) for r in rec]
        rarr = (_c.c_void_p * max(1, len(rec)))(*[_c.addressof(b) for b in rbufs])
        rlens = (_c.c_int * max(1, len(rec)))(*[len(r) for r in rec])
        keep += [ids, obufs, oarr, olens, rbufs, rarr, rlens]
        rx[i] = sg.RxGroup(len(orig), _c.addressof(ids), oarr, olens, len(rec), rarr, rlens)
    return keep, rx


@pytest.mark.gpu
def test_device_delivery_without_a_callback():
    """on_packet = NULL with delivery 1: the same count, the kernel and both copies still run (the same
    D2H bytes as with a callback), nothing is delivered."""
    import shorthair_amd as sh
    from shorthair_amd import groups as sg
    ora = po.oracle()
    groups, _ = _workload()
    rx = _receive(groups, [opk.tx_group(ora, m, pk) for m, pk in groups], seed=15)
    want_n, _ = _oracle_deliveries(ora, rx)
    keep, arr = _rx_array(sg, rx)
    assert sg.set_framing(0) == 0 and sg.set_delivery(0) == 0
    try:
        for framing in (0, 1):
            sg.set_framing(framing)
            sg.set_delivery(1)
            n, delivered, stats, d2h = _recover(sh, sg, rx)
            assert n == want_n and delivered
            l0, t0 = sh.groups_stats(), sg.traffic()
            rc = sh.lib.shorthair_recover_groups(arr, len(rx), sg.ON_PACKET(), None)
            l1, t1 = sh.groups_stats(), sg.traffic()
            assert rc == want_n
            assert (l1[0] - l0[0], l1[1] - l0[1]) == stats and t1[1] - t0[1] == d2h
            sg.set_delivery(0)
            assert sh.lib.shorthair_recover_groups(arr, len(rx), sg.ON_PACKET(), None) == want_n
    finally:
        sg.set_delivery(0)
        sg.set_framing(0)
    del keep


@pytest.mark.gpu
def test_device_delivery_over_several_chunks():
    """Headline-sized groups (k = 200, m = 32, B = 1400) span several double-buffered chunks, each with
    its own payload total: the second-phase copies of one chunk run beside the next chunk's kernels, and
    delivery 1 gives delivery 0's callbacks on both framing routes, a sample of groups the oracle's."""
    import shorthair_amd as sh
    from shorthair_amd import groups as sg
    ora = po.oracle()
    nprng = np.random.default_rng(19)
    G, k, m = 300, 200, 32
    groups = []
    for _ in range(G):
        lens = [int(v) for v in nprng.integers(0, 1399, size=k)]
        lens[0] = 1398  # B = 1400
        whole = nprng.integers(0, 256, size=sum(lens), dtype=np.uint8).tobytes()
        cuts = np.concatenate([[0], np.cumsum(lens)])
        groups.append((m, [whole[cuts[i]:cuts[i + 1]] for i in range(k)]))
    rng = random.Random(4)
    assert sg.set_framing(0) == 0 and sg.set_delivery(0) == 0
    try:
        recs = sg.encode_groups(groups)
        rx = []
        for (_, pk), rec in zip(groups, recs):
            e = rng.randint(1, m)
            lost = set(rng.sample(range(k), e))
            orig = [(i, pk[i]) for i in range(k) if i not in lost]
            rng.shuffle(orig)
            rx.append((orig, rng.sample(rec, e)))
        host = _recover(sh, sg, rx)
        assert host[0] == G and host[2][0] >= 2       # several chunks
        for framing in (0, 1):
            sg.set_framing(framing)
            sg.set_delivery(1)
            dev = _recover(sh, sg, rx)
            assert dev[:3] == host[:3], framing
            assert dev[3] < host[3]
        for gi in (0, 151, G - 1):
            assert [(pid, p) for g, pid, p in host[1] if g == gi] == opk.rx_group(ora, *rx[gi])
    finally:
        sg.set_delivery(0)
        sg.set_framing(0)


@pytest.mark.gpu
def test_device_delivery_region_survives_a_larger_next_chunk():
    """Four chunks of one bucket (k = 200, m = 32, B = 1400: 154 groups per chunk), so each slot is reused
    while its previous chunk's `late` step is pending. The first two chunks carry short payloads and
    lose one original per group; the last two carry full payloads, so their inputs are several times the
    first two's inputs plus outputs. A chunk's pinned delivery-1 region (total, len[], rows, packed
    payloads) is read after the slot's next chunk has been prepared, so it must lie behind the largest
    chunk's layout, not the chunk's own: delivery 1 gives delivery 0's callbacks on both framing routes."""
    import shorthair_amd as sh
    from shorthair_amd import groups as sg
    ora = po.oracle()
    nprng = np.random.default_rng(23)
    rng = random.Random(5)
    per, k, m = 154, 200, 32
    G = 3 * per + 60
    groups, rx_e = [], []
    for g in range(G):
        short = g < 2 * per
        lens = [int(v) for v in nprng.integers(0, 21, size=k)] if short else [1398] * k
        lens[0] = 1398  # B = 1400
        whole = nprng.integers(0, 256, size=sum(lens), dtype=np.uint8).tobytes()
        cuts = np.concatenate([[0], np.cumsum(lens)])
        groups.append((m, [whole[cuts[i]:cuts[i + 1]] for i in range(k)]))
        rx_e.append(1 if short else rng.randint(1, m))
    assert sg.set_framing(0) == 0 and sg.set_delivery(0) == 0
    try:
        recs = sg.encode_groups(groups)
        rx = []
        for (_, pk), rec, e in zip(groups, recs, rx_e):
            lost = set(rng.sample(range(1, k), e))  # (the full-size original stays: small chunk inputs)
            orig = [(i, pk[i]) for i in range(k) if i not in lost]
            rng.shuffle(orig)
            rx.append((orig, rng.sample(rec, e)))
        host = _recover(sh, sg, rx)
        assert host[0] == G and host[2] == (4, G)     # four chunks, a launch each
        for framing in (0, 1):
            sg.set_framing(framing)
            sg.set_delivery(1)
            dev = _recover(sh, sg, rx)
            assert dev[:3] == host[:3], framing
        for gi in (0, per, 2 * per, G - 1):
            assert [(pid, p) for g, pid, p in host[1] if g == gi] == opk.rx_group(ora, *rx[gi])
    finally:
        sg.set_delivery(0)
        sg.set_framing(0)
