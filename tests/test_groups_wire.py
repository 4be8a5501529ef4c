"""Recovery packets emitted on the GPU (include/shorthair_groups.h: shorthair_groups_set_wire(1)).

Wire route 1 builds the "[k+y][k-1][m-1][block]" records of every k >= 2 bucket in device memory and
brings them back whole; every group's out bytes, m_out, out_stride, the launches and the H2D traffic
must equal wire route 0's on both framing routes, the bytes the oracle's (oracle/packets.py on the CPU
oracle), and the D2H traffic is exactly the records.
"""
import ctypes

import numpy as np
import pytest

from oracle import packets as opk
from oracle import pyoracle as po

BIG_G, BIG_K, BIG_M = 330, 200, 32  # 324,800 device bytes per group: three 48 MB chunks


# ---------------------------------------------------------------- CPU

def test_set_wire_returns_previous_and_rejects_others():
    from shorthair_amd import groups as sg
    import shorthair_amd as sh
    f = sh.lib.shorthair_groups_set_wire
    try:
        assert f(0) == 0          # the default
        assert f(1) == 0 and f(1) == 1 and f(0) == 1
        for bad in (2, -1, 3, 1 << 20):
            assert f(bad) == -1
            assert f(0) == 0      # a rejected argument changes nothing
        assert sg.set_wire(1) == 0 and sg.set_wire(0) == 1
        with pytest.raises(ValueError):
            sg.set_wire(2)
    finally:
        f(0)


# ---------------------------------------------------------------- workload

def _payload(rng, n):
    return rng.integers(0, 256, size=int(n), dtype=np.uint8).tobytes()


def _group(rng, k, m, largest, short=None):
    """k payloads of 0..short bytes (largest when None), one of them `largest` bytes long."""
    lens = [int(v) for v in rng.integers(0, (largest if short is None else short) + 1, size=k)]
    lens[int(rng.integers(0, k))] = largest
    return (m, [_payload(rng, n) for n in lens])


def _workload():
    """(groups, indices of a sample to check against the oracle)."""
    rng = np.random.default_rng(2025)
    groups, sample = [], []
    groups.append((3, [_payload(rng, 40)]))                             # k = 1: stays on the host
    groups += [_group(rng, 10, 4, 254) for _ in range(5)]               # uniform bucket: k = 10, m = 4, B = 256
    groups += [_group(rng, 17 + (i * 5) % 12, 4, 1350, 64) for i in range(16)]  # mixed k, one compiled K = 28
    groups += [_group(rng, k, 1, 100) for k in (5, 5, 9)]               # m = 1
    groups += [_group(rng, 20, 10, 134) for _ in range(6)]              # tile kernels: (20, 10, 136)
    groups.append((60, [_payload(rng, 30) for _ in range(250)]))        # m truncated to 256 - k = 6
    sample = list(range(len(groups)))
    big = len(groups)
    groups += [_group(rng, BIG_K, BIG_M, 1398, 16) for _ in range(BIG_G)]  # one bucket of three chunks
    sample += [big, big + 154, big + BIG_G - 1]
    return groups, sample


def _encode(sh, groups):
    """shorthair_encode_groups through ctypes, keeping what the binding's encode_groups drops: per group
    (out bytes up to m_out * out_stride, m_out, out_stride)."""
    from shorthair_amd import groups as sg
    keep, tx, outs = [], (sg.TxGroup * len(groups))(), []
    for i, (m, packets) in enumerate(groups):
        k = len(packets)
        bufs = [ctypes.create_string_buffer(p, max(1, len(p))) for p in packets]
        arr = (ctypes.c_void_p * k)(*[ctypes.addressof(b) for b in bufs])
        lens = (ctypes.c_ushort * k)(*[len(p) for p in packets])
        cap = sg.recovery_packet_bytes(k, [len(p) for p in packets]) * min(m, 256 - k)
        out = ctypes.create_string_buffer(cap)
        keep += [bufs, arr, lens]
        outs.append(out)
        tx[i] = sg.TxGroup(k, m, arr, lens, ctypes.addressof(out), cap, 0, 0)
    assert sh.lib.shorthair_encode_groups(tx, len(groups)) == 0
    return [(outs[i].raw[:tx[i].m_out * tx[i].out_stride], tx[i].m_out, tx[i].out_stride) for i in range(len(groups))]


def test_workload_has_every_kind_of_bucket():
    """The arithmetic of the workload on the CPU: the buckets the issue names, and a bucket whose groups
    cannot fit two 48 MB chunks."""
    groups, sample = _workload()
    ks = [len(pk) for _, pk in groups]
    assert ks.count(1) == 1 and any(m == 1 and len(pk) > 1 for m, pk in groups)
    assert len({len(pk) for m, pk in groups if m == 4 and len(pk) >= 17}) > 1
    per_group = (BIG_K + BIG_M) * 1400
    assert ks.count(BIG_K) == BIG_G and BIG_G * per_group > 2 * (48 << 20)
    assert all(opk.roundup8(2 + max(len(p) for p in pk)) == 1400 for m, pk in groups if len(pk) == BIG_K)
    assert len(sample) >= 30


# ---------------------------------------------------------------- GPU

@pytest.mark.gpu
def test_device_wire_matches_host_wire_and_oracle():
    import shorthair_amd as sh
    from shorthair_amd import groups as sg
    ora = po.oracle()
    groups, sample = _workload()
    assert sh.path(20, 10, 136) == "tile" and sh.path(28, 4, 1352) == "fixed"
    # what wire route 1 must bring back: the records of every k >= 2 group, and nothing else
    records = 0
    for m, pk in groups:
        if len(pk) >= 2:
            records += min(m, 256 - len(pk)) * (3 + opk.roundup8(2 + max(len(p) for p in pk)))
    assert sg.set_framing(0) == 0 and sg.set_wire(0) == 0
    try:
        res = {}
        for framing in (0, 1):
            for wire in (0, 1):
                sg.set_framing(framing)
                sg.set_wire(wire)
                t0, s0 = sg.traffic(), sh.groups_stats()
                out = _encode(sh, groups)
                t1, s1 = sg.traffic(), sh.groups_stats()
                res[framing, wire] = (out, (s1[0] - s0[0], s1[1] - s0[1]), t1[0] - t0[0], t1[1] - t0[1])
            assert sh.lib.shorthair_groups_set_wire(2) == -1  # rejected: the route stays 1
            assert sg.set_wire(0) == 1
        print("launches/groups, h2d, d2h per (framing, wire):", {k: v[1:] for k, v in res.items()})
        for framing in (0, 1):
            host, dev = res[framing, 0], res[framing, 1]
            bad = [i for i in range(len(groups)) if dev[0][i] != host[0][i]]
            assert not bad, (framing, bad[:8])            # out bytes, m_out and out_stride of every group
            assert dev[1] == host[1]                      # the same launches over the same groups
            assert dev[1][0] >= 3 + 5 and dev[1][1] == sum(1 for _, pk in groups if len(pk) >= 2)
            assert dev[2] == host[2] > 0                  # the same H2D traffic
            assert dev[3] == records                      # D2H: exactly the records
            assert host[3] == records - 3 * sum(min(m, 256 - len(pk)) for m, pk in groups if len(pk) >= 2)
        for i in sample:
            m, pk = groups[i]
            want = opk.tx_group(ora, m, pk)
            for framing in (0, 1):
                raw, m_out, stride = res[framing, 1][0][i]
                assert m_out == len(want) and stride == len(want[0]), i
                assert raw == b"".join(want), (i, framing)
    finally:
        sg.set_framing(0)
        sg.set_wire(0)
