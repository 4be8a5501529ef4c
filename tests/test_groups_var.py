"""Packet groups with mixed k through one var-k launch per (K, m, B) bucket
(include/shorthair_groups.h): groups that the codec would code with the same compiled kernel share a
launch, wire bytes and delivery order stay the reference's (oracle/packets.py on the CPU oracle), and
shorthair_groups_stats shows the merge.
"""
import random

import numpy as np
import pytest

from oracle import packets as opk
from oracle import pyoracle as po

M, LARGEST = 4, 254  # B = roundup8(2 + 254) = 256


def _tx_groups():
    rng = random.Random(41)
    nprng = np.random.default_rng(41)
    ks = [17 + (i * 5) % 12 for i in range(37)] + [10, 10, 10]
    rng.shuffle(ks)
    groups = []
    for k in ks:
        lens = nprng.integers(0, LARGEST + 1, size=k)
        lens[rng.randrange(k)] = LARGEST
        groups.append((M, [nprng.integers(0, 256, size=int(n), dtype=np.uint8).tobytes() for n in lens]))
    return ks, groups


@pytest.mark.gpu
def test_mixed_k_groups_share_var_launches():
    import shorthair_amd as sh
    from shorthair_amd import groups as sg
    ora = po.oracle()
    ks, groups = _tx_groups()
    assert len(groups) == 40 and set(ks) == set(range(17, 29)) | {10}
    B = 256
    # bucket keys: the compiled K when (k, m, B) runs a compile-time kernel (only (28, 4) has m = 4)
    keys = {(28 if sh.path(k, M, B) == "fixed" else k, M, B) for k in ks}
    assert keys == {(28, M, B), (10, M, B)} and len(keys) < len(set(ks))

    l0, g0 = sh.groups_stats()
    recs = sg.encode_groups(groups)
    l1, g1 = sh.groups_stats()
    assert l1 - l0 == len(keys) and g1 - g0 == len(groups)
    expect = [opk.tx_group(ora, m, pk) for m, pk in groups]
    assert recs == expect

    rng = random.Random(7)
    rx, want = [], []
    for (m, pk), rec in zip(groups, recs):
        k = len(pk)
        e = rng.randint(1, min(k, len(rec)))
        lost = set(rng.sample(range(k), e))
        orig = [(i, pk[i]) for i in range(k) if i not in lost]
        rng.shuffle(orig)
        got = rng.sample(rec, rng.randint(e, len(rec)))
        rx.append((orig, got))
        want.append(opk.rx_group(ora, orig, got))
    n, delivered = sg.recover_groups(rx)
    l2, g2 = sh.groups_stats()
    assert n == len(groups)
    assert l2 - l1 == len(keys) and g2 - g1 == len(groups)
    by_group = {}
    for g, pid, p in delivered:
        by_group.setdefault(g, []).append((pid, p))
    for gi in range(len(groups)):
        assert by_group.get(gi) == want[gi], gi
