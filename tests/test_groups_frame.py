"""Packet groups framed on the GPU (include/shorthair_groups.h: shorthair_groups_set_framing(1)).

Route 1 sends only the payload bytes over PCIe and lets shorthair_frame_batch build the code blocks
in device memory; wire bytes, deliveries, return values and launch counts must equal route 0's and
the oracle's (oracle/packets.py on the CPU oracle), and shorthair_groups_traffic must show the
saving on short payloads.
"""
import random

import numpy as np
import pytest

from oracle import packets as opk
from oracle import pyoracle as po


# ---------------------------------------------------------------- CPU

def test_set_framing_returns_previous_and_rejects_others():
    from shorthair_amd import groups as sg
    import shorthair_amd as sh
    f = sh.lib.shorthair_groups_set_framing
    try:
        assert f(0) == 0          # the default
        assert f(1) == 0 and f(1) == 1 and f(0) == 1
        for bad in (2, -1, 3, 1 << 20):
            assert f(bad) == -1
            assert f(0) == 0      # a rejected argument changes nothing
        assert sg.set_framing(1) == 0 and sg.set_framing(0) == 1
        with pytest.raises(ValueError):
            sg.set_framing(2)
    finally:
        f(0)


def test_traffic_is_zero_before_any_call():
    """A fresh process: shorthair_groups_traffic returns 0 and both counters are zero; k = 1 groups
    (host only) leave them there."""
    import subprocess
    import sys
    import os
    root = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    code = ("import ctypes; import shorthair_amd as sh; from shorthair_amd import groups as sg; "
            "a, b = ctypes.c_longlong(7), ctypes.c_longlong(7); "
            "assert sh.lib.shorthair_groups_traffic(ctypes.byref(a), ctypes.byref(b)) == 0; "
            "assert (a.value, b.value) == (0, 0); assert sg.traffic() == (0, 0); "
            "assert sh.lib.shorthair_groups_traffic(None, None) == 0; "
            "assert sg.encode_groups([(2, [b'abc'])]) == [[b'\\x01\\x00abc'] * 2]; "
            "assert sg.traffic() == (0, 0); print('ok')")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, cwd=root)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-800:]


# ---------------------------------------------------------------- workload

SHORT_K, SHORT_M, SHORT_LONG = 30, 4, 1350  # short-payload groups: B = roundup8(2 + 1350) = 1352


def _payload(nprng, n):
    return nprng.integers(0, 256, size=int(n), dtype=np.uint8).tobytes()


def _short_groups(nprng, count=10):
    """Many short payloads (0..64 bytes) and one long one per group: B >> the mean length."""
    groups = []
    for _ in range(count):
        lens = [int(v) for v in nprng.integers(0, 65, size=SHORT_K)]
        lens[int(nprng.integers(0, SHORT_K))] = SHORT_LONG
        groups.append((SHORT_M, [_payload(nprng, n) for n in lens]))
    return groups


def _workload():
    """About 40 groups: k = 1, a uniform bucket, a mixed-k bucket, m = 1, full-size payloads, a
    zero-length payload, and the short-payload groups. Returns (groups, indices of the short ones)."""
    nprng = np.random.default_rng(2024)
    groups = []
    groups.append((3, [_payload(nprng, 40)]))                      # k = 1
    groups.append((1, [b""]))                                      # k = 1, empty payload
    for _ in range(5):                                             # uniform bucket: k = 10, m = 4, B = 256
        lens = [int(v) for v in nprng.integers(1, 255, size=10)]
        lens[3] = 254
        groups.append((4, [_payload(nprng, n) for n in lens]))
    for i in range(16):                                          # mixed-k bucket (K = 28, m = 4, B = 256)
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
    groups += _short_groups(nprng)
    groups += [(4, [_payload(nprng, n) for n in [254] + [7] * 20])]  # one more k for the mixed bucket
    order = list(range(len(groups)))
    random.Random(5).shuffle(order)
    shuffled = [groups[i] for i in order]
    short = [order.index(i) for i in short]
    return shuffled, sorted(short)


def _receive(groups, recs, seed):
    """One receive pattern per group: (originals, recovery packets) in arrival order."""
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


def test_workload_bounds_are_far_apart():
    """The arithmetic of the traffic check, on the CPU: what route 1 may copy for the short-payload
    groups is a small fraction of what route 0 must."""
    groups, short = _workload()
    assert 38 <= len(groups) <= 45 and len(short) == 10
    ks = [len(pk) for _, pk in groups]
    assert ks.count(1) == 2 and any(m == 1 and len(pk) > 1 for m, pk in groups)
    assert any(len(p) == 0 for _, pk in groups for p in pk)
    sel = [groups[i] for i in short]
    for m, pk in sel:
        assert len(pk) == SHORT_K and opk.roundup8(2 + max(len(p) for p in pk)) == 1352
        assert sorted(len(p) for p in pk)[-2] <= 64
    payload = sum(len(p) for _, pk in sel for p in pk)
    blocks = sum(len(pk) for _, pk in sel)
    route1_max = payload + 32 * blocks + 4096 * 1
    route0_min = blocks * 1352
    assert route0_min == 405600 and route1_max < 40000 and 8 * route1_max < route0_min


# ---------------------------------------------------------------- GPU

@pytest.mark.gpu
def test_device_framing_matches_host_framing_and_oracle():
    import shorthair_amd as sh
    from shorthair_amd import groups as sg
    ora = po.oracle()
    groups, short = _workload()
    expect = [opk.tx_group(ora, m, pk) for m, pk in groups]
    rx = _receive(groups, expect, seed=13)
    want_n, want = _oracle_deliveries(ora, rx)
    assert sg.set_framing(0) == 0
    try:
        res = {}
        for route in (0, 1):
            sg.set_framing(route)
            l0, g0 = sh.groups_stats()
            recs = sg.encode_groups(groups)
            l1, g1 = sh.groups_stats()
            n, delivered = sg.recover_groups(rx)
            l2, g2 = sh.groups_stats()
            res[route] = (recs, n, delivered, (l1 - l0, g1 - g0, l2 - l1, g2 - g1))
        assert res[1][0] == expect and res[0][0] == expect
        assert res[1][1] == want_n == res[0][1]
        assert res[1][2] == res[0][2]                    # the same deliveries in the same order
        for route in (0, 1):                             # and per group the oracle's: ids, payloads, order
            by_group = {}
            for g, pid, p in res[route][2]:
                by_group.setdefault(g, []).append((g, pid, p))
            assert sorted(by_group) == sorted({g for g, _, _ in want})
            assert [d for g in sorted(by_group) for d in by_group[g]] == want
        assert res[1][3] == res[0][3]                    # the same launches over the same groups
        assert res[0][3][1] == sum(1 for _, pk in groups if len(pk) >= 2)

        # traffic on the short-payload groups alone
        sel = [groups[i] for i in short]
        sel_rx = [rx[i] for i in short]
        blocks = sum(len(pk) for _, pk in sel)
        tx_payload = sum(len(p) for _, pk in sel for p in pk)
        rx_payload = 0
        for (m, pk), (orig, rec) in zip(sel, sel_rx):
            rx_payload += sum(len(p) for _, p in orig) + (len(pk) - len(orig)) * 1352
        delta = {}
        for route in (0, 1):
            sg.set_framing(route)
            t0, l0 = sg.traffic(), sh.groups_stats()[0]
            assert sg.encode_groups(sel) == [expect[i] for i in short]
            t1, l1 = sg.traffic(), sh.groups_stats()[0]
            n, _ = sg.recover_groups(sel_rx)
            t2, l2 = sg.traffic(), sh.groups_stats()[0]
            assert n == len(sel)
            delta[route] = (t1[0] - t0[0], l1 - l0, t2[0] - t1[0], l2 - l1, t1[1] - t0[1], t2[1] - t1[1])
        print("h2d/launches/d2h per route:", delta)
        h2d_tx, chunks_tx, h2d_rx, chunks_rx = delta[1][:4]
        assert 0 < h2d_tx <= tx_payload + 32 * blocks + 4096 * chunks_tx
        assert 0 < h2d_rx <= rx_payload + 32 * blocks + 4096 * chunks_rx
        assert delta[0][0] >= blocks * 1352 and delta[0][2] >= blocks * 1352
        assert delta[1][4] == delta[0][4] > 0 and delta[1][5] == delta[0][5] > 0  # outputs: the same D2H
    finally:
        sg.set_framing(0)


@pytest.mark.gpu
@pytest.mark.parametrize("mixed", [False, True], ids=["uniform", "mixed_k"])
def test_device_framing_over_several_chunks(mixed):
    """Headline-sized groups (k <= 200, m = 32, B = 1400) span several double-buffered chunks whose
    slot layouts all differ (the payload lengths do): route 1 gives route 0's bytes and deliveries,
    chunk for chunk, and a sample of groups the oracle's."""
    import shorthair_amd as sh
    from shorthair_amd import groups as sg
    ora = po.oracle()
    nprng = np.random.default_rng(17 + mixed)
    G, m = 300, 32
    ks = [int(v) for v in nprng.integers(150, 201, size=G)] if mixed else [200] * G
    groups = []
    for k in ks:
        lens = [int(v) for v in nprng.integers(0, 1399, size=k)]
        lens[0] = 1398  # B = 1400
        whole = nprng.integers(0, 256, size=sum(lens), dtype=np.uint8).tobytes()
        cuts = np.concatenate([[0], np.cumsum(lens)])
        groups.append((m, [whole[cuts[i]:cuts[i + 1]] for i in range(k)]))
    rng = random.Random(3)
    assert sg.set_framing(0) == 0
    try:
        res = {}
        for route in (0, 1):
            sg.set_framing(route)
            l0 = sh.groups_stats()[0]
            recs = sg.encode_groups(groups)
            l1 = sh.groups_stats()[0]
            if route == 0:
                rx = []
                for k, (_, pk), rec in zip(ks, groups, recs):
                    lost = set(rng.sample(range(k), m))
                    orig = [(i, pk[i]) for i in range(k) if i not in lost]
                    rng.shuffle(orig)
                    rx.append((orig, rng.sample(rec, m)))
            n, delivered = sg.recover_groups(rx)
            l2 = sh.groups_stats()[0]
            res[route] = (recs, n, delivered, l1 - l0, l2 - l1)
        assert res[0][3] >= 2 and res[0][4] >= 2      # several chunks each way
        assert res[1] == res[0]
        assert res[1][1] == G and len(res[1][2]) == G * m
        for gi in (0, 151, G - 1):
            assert res[1][0][gi] == opk.tx_group(ora, m, groups[gi][1])
            assert [(pid, p) for g, pid, p in res[1][2] if g == gi] == opk.rx_group(ora, *rx[gi])
    finally:
        sg.set_framing(0)


@pytest.mark.gpu
def test_loopback_statistics_equal_on_both_routes():
    from shorthair_amd import groups as sg
    from shorthair_amd import loopback as lb
    assert sg.set_framing(0) == 0
    try:
        host = lb.run(160, batch=4)
        sg.set_framing(1)
        dev = lb.run(160, batch=4)
    finally:
        sg.set_framing(0)
    assert host.bad == [] and host.recovered == host.expected_recovered > 0
    assert vars(dev) == vars(host)
