"""Exact PCIe byte counts of the packet-group calls (include/shorthair_groups.h).

The route-against-route tests bound shorthair_groups_traffic; this one pins it. For both framing
routes, both deliveries and two small calls (uniform buckets, m = 1, k = 1; one mixed-k bucket) the
H2D and D2H deltas equal the sums over the call's buckets of what the slot layout says a chunk
ships, so a path that always shipped first[], or a whole slot, fails here. Launches,
wire bytes and deliveries are checked against the oracle (oracle/packets.py) on all four settings.
"""
import random

import numpy as np
import pytest

from oracle import packets as opk
from oracle import pyoracle as po

B = 128  # roundup8(2 + 126)


def up16(x):
    return (x + 15) & ~15


def _group(nprng, rng, k, m):
    """k payloads: one of 126 bytes, one empty (k >= 2), the others 0..126 bytes."""
    lens = [int(v) for v in nprng.integers(0, 127, size=k)]
    a, b = rng.sample(range(k), 2)
    lens[a], lens[b] = 126, 0
    return m, [nprng.integers(0, 256, size=n, dtype=np.uint8).tobytes() for n in lens]


def _calls():
    nprng, rng = np.random.default_rng(17), random.Random(17)
    a = [_group(nprng, rng, 5, 2) for _ in range(3)] + [_group(nprng, rng, 3, 1) for _ in range(2)]
    a.insert(2, (2, [nprng.integers(0, 256, size=126, dtype=np.uint8).tobytes()]))  # k = 1
    b = [_group(nprng, rng, k, 4) for k in (17, 22, 28, 28, 19)]
    return a, b


def _receive(groups, recs, seed):
    """Each k >= 2 group loses e originals (e = 1 for the first of a call, so some e < emax), the rest
    arrive shuffled with exactly e recovery packets; a k = 1 group arrives as its recovery packet."""
    rng = random.Random(seed)
    rx, first = [], True
    for (m, pk), rec in zip(groups, recs):
        k = len(pk)
        if k == 1:
            rx.append(([], rec[:1]))
            continue
        e = 1 if first else rng.randint(1, min(k, m))
        first = False
        lost = set(rng.sample(range(k), e))
        orig = [(i, pk[i]) for i in range(k) if i not in lost]
        rng.shuffle(orig)
        rx.append((orig, rng.sample(rec, e)))
    return rx


def _buckets(groups, path):
    """{(k or "mixed", m): [group index]} of a call's k >= 2 groups, by the library's bucket key (K, m, B):
    K is the compiled kernel's k when path(k, m, B) is "fixed" and m >= 2, else k itself. Only one compiled
    kernel has m = 4 (28, 4), so the fixed groups of one m share a bucket; a bucket with more than one
    distinct k is "mixed"."""
    keyed = {}
    for g, (m, pk) in enumerate(groups):
        if len(pk) >= 2:
            fixed = m >= 2 and path(len(pk), m, B) == "fixed"
            keyed.setdefault(("fixed" if fixed else len(pk), m), []).append(g)
    out = {}
    for (key, m), gs in keyed.items():
        ks = {len(groups[g][1]) for g in gs}
        out["mixed" if len(ks) > 1 else ks.pop(), m] = gs
    return out


def _expect_tx(groups, framing, path):
    h2d = d2h = 0
    for (key, m), gs in _buckets(groups, path).items():
        gn, nb = len(gs), sum(len(groups[g][1]) for g in gs)
        F = 4 * (gn + 1) if key == "mixed" else 0
        pay = sum(len(p) for g in gs for p in groups[g][1])
        h2d += nb * B + F if framing == 0 else up16(12 * nb + F) + pay
        d2h += gn * m * B
    return h2d, d2h


def _expect_rx(groups, rx, want, framing, delivery, path):
    h2d = d2h = 0
    for (key, m), gs in _buckets(groups, path).items():
        gn, nb = len(gs), sum(len(groups[g][1]) for g in gs)
        F = 4 * (gn + 1) if key == "mixed" else 0
        emax = min(max(len(groups[g][1]) for g in gs), m)
        pay = sum(len(p) for g in gs for _, p in rx[g][0]) + B * sum(len(rx[g][1]) for g in gs)
        h2d += nb * B + nb + F if framing == 0 else up16(14 * nb + F) + pay
        if m == 1:
            d2h += gn * B
        elif delivery == 0:
            d2h += gn * emax * B + gn * emax
        else:
            d2h += 8 + 5 * gn * emax + sum(len(p) for g, _, p in want if g in gs)
    return h2d, d2h


def _check_workload(a, b, path):
    """The workload is the one the formulas assume."""
    assert [(len(pk), m) for m, pk in a] == [(5, 2), (5, 2), (1, 2), (5, 2), (3, 1), (3, 1)]
    assert [(len(pk), m) for m, pk in b] == [(17, 4), (22, 4), (28, 4), (28, 4), (19, 4)]
    for m, pk in a + b:
        assert max(len(p) for p in pk) == 126
        assert len(pk) == 1 or min(len(p) for p in pk) == 0
    assert set(_buckets(a, path)) == {(5, 2), (3, 1)} and set(_buckets(b, path)) == {("mixed", 4)}


@pytest.mark.gpu
def test_traffic_is_exactly_what_the_layout_ships():
    import shorthair_amd as sh
    from shorthair_amd import groups as sg
    ora = po.oracle()
    calls = _calls()
    _check_workload(*calls, sh.path)
    assert all(sh.path(len(pk), 4, B) == "fixed" for _, pk in calls[1])
    assert sh.path(5, 2, B) == "tile"
    work = []
    for ci, groups in enumerate(calls):
        recs = [opk.tx_group(ora, m, pk) for m, pk in groups]
        rx = _receive(groups, recs, seed=23 + ci)
        es = [len(pk) - len(orig) for (m, pk), (orig, _) in zip(groups, rx) if len(pk) >= 2]
        assert all(e >= 1 for e in es) and 1 in es and max(es) >= 2
        want = [(g, pid, p) for g, (orig, rec) in enumerate(rx) for pid, p in opk.rx_group(ora, orig, rec)]
        work.append((groups, recs, rx, want))
    assert sg.set_framing(0) == 0 and sg.set_delivery(0) == 0
    try:
        for framing in (0, 1):
            for delivery in (0, 1):
                sg.set_framing(framing)
                sg.set_delivery(delivery)
                for ci, (groups, recs, rx, want) in enumerate(work):
                    key = (framing, delivery, "AB"[ci])
                    coded = sum(1 for _, pk in groups if len(pk) >= 2)
                    launches = len(_buckets(groups, sh.path))
                    s0, t0 = sh.groups_stats(), sg.traffic()
                    got = sg.encode_groups(groups)
                    s1, t1 = sh.groups_stats(), sg.traffic()
                    n, delivered = sg.recover_groups(rx)
                    s2, t2 = sh.groups_stats(), sg.traffic()
                    tx = (t1[0] - t0[0], t1[1] - t0[1])
                    rxb = (t2[0] - t1[0], t2[1] - t1[1])
                    print(key, "tx h2d/d2h", tx, "rx h2d/d2h", rxb)
                    assert got == recs, key
                    assert n == len(groups), key
                    by_group = sorted(delivered, key=lambda d: d[0])  # stable: per group, delivery order
                    assert by_group == want, key
                    assert (s1[0] - s0[0], s1[1] - s0[1]) == (launches, coded), key
                    assert (s2[0] - s1[0], s2[1] - s1[1]) == (launches, coded), key
                    assert tx == _expect_tx(groups, framing, sh.path), key
                    assert rxb == _expect_rx(groups, rx, want, framing, delivery, sh.path), key
    finally:
        sg.set_delivery(0)
        sg.set_framing(0)
