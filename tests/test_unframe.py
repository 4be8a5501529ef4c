"""Device-resident delivery of recovered blocks (include/shorthair_unframe.h: shorthair_unframe_batch).

Expected values come from the delivery rule of RecoverGroup (Shorthair.cpp:741-756) restated in numpy
below -- read the u16 prefix, deliver `data + 2, len` when len <= B - 2 -- with the packing the header
specifies, and, for the compositions with the codec calls, from oracle/packets.py::rx_group on the CPU
oracle -- never from the library under test.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import packets as opk
from oracle import pyoracle as po

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
CANARY = 0xC3  # around d_payload, and under every byte of it that must stay unwritten
PAD = 4096
INT_MAX = 2 ** 31 - 1


def unframe_rule(B, groups, emax, stride, src, count, capacity):
    """src: the bytes from d_out on. Returns (len[slots], off[slots + 1], payload[capacity] over a
    CANARY background, errors); capacity None: lengths and offsets only (payload None, errors of the
    counts alone)."""
    slots = groups * emax
    length = np.full(slots, -1, np.int32)
    off = np.zeros(slots + 1, np.int64)
    pay = np.full(capacity, CANARY, np.uint8) if capacity is not None else None
    errors, pos = 0, 0
    for g in range(groups):
        c = emax if count is None else int(count[g])
        if c < -1 or c > emax:
            errors += 1
            c = 0
        for i in range(emax):
            s = g * emax + i
            off[s] = pos
            if i >= c:
                continue
            b = (g * stride + i) * B
            p = int(src[b]) | (int(src[b + 1]) << 8)
            if p > B - 2:
                length[s] = -2
                continue
            length[s] = p
            if capacity is None:
                pass
            elif p > 0 and pos + p > capacity:
                errors += 1
            else:
                pay[pos:pos + p] = src[b + 2:b + 2 + p]
            pos += p
    off[slots] = pos
    return length, off, pay, errors


def put_prefix(blocks, j, p):
    blocks[j, 0], blocks[j, 1] = p & 0xFF, p >> 8


def build_case(B, groups, emax, seed, stride=None, with_count=True):
    """Random bytes everywhere -- behind every payload and in the slots past each group's count, whose
    prefixes look valid -- then prefixes: the special lengths first, random ones after. Counts cover 0,
    emax and values between."""
    stride = emax if stride is None else stride
    rng = np.random.default_rng(seed)
    blocks = rng.integers(0, 256, size=(groups * stride, B), dtype=np.uint8)
    top = min(B - 2, 65535)
    if with_count:
        count = rng.integers(0, emax + 1, size=groups).astype(np.int32)
        count[0] = emax
        if groups > 1:
            count[1] = 0
        if groups > 2:
            count[2] = (emax + 1) // 2
    else:
        count = None
    special = []
    for p in (0, 1, 5, 6, 7, B - 3, B - 2):
        if 0 <= p <= top and p not in special:
            special.append(p)
    n = 0
    for g in range(groups):
        c = emax if count is None else int(count[g])
        for i in range(emax):
            if i < c:
                p = special[n] if n < len(special) else int(rng.integers(0, top + 1))
                n += 1
            else:
                p = int(rng.integers(0, top + 1))  # stale, but it looks valid
            put_prefix(blocks, g * stride + i, p)
    return blocks, count


@pytest.fixture(scope="module")
def sh():
    import torch
    import shorthair_amd
    assert shorthair_amd.cauchy_256_init() == 0
    torch.cuda.init()
    return shorthair_amd


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.size == 0:
        return torch.zeros(16, dtype=torch.uint8, device="cuda")
    return torch.from_numpy(a).cuda()


def run_unframe(sh, B, groups, emax, stride, src, count, capacity, misalign=0, src_skip=0, null_payload=False):
    """Unframes on the GPU into a guarded buffer whose base is = misalign (mod 16); `src` is the whole
    source array and d_out starts src_skip bytes into it. Checks both canaries and that the source is
    unchanged; returns (rc, len, off, payload[capacity])."""
    import torch
    slots = groups * emax
    dsrc = _dev(src)
    dcount = _dev(count) if count is not None else None
    buf = torch.full((PAD + 16 + capacity + PAD,), CANARY, dtype=torch.uint8, device="cuda")
    start = PAD + (misalign - (buf.data_ptr() + PAD)) % 16
    assert (buf.data_ptr() + start) % 16 == misalign
    doff = torch.full((slots + 1,), -7, dtype=torch.int64, device="cuda")
    dlen = torch.full((max(slots, 1),), -7, dtype=torch.int32, device="cuda")
    scratch = torch.zeros(sh.unframe_scratch_bytes(groups, emax), dtype=torch.uint8, device="cuda")
    rc = sh.lib.shorthair_unframe_batch(B, groups, emax, stride, dsrc.data_ptr() + src_skip,
                                        dcount.data_ptr() if dcount is not None else None,
                                        None if null_payload else buf.data_ptr() + start, capacity,
                                        doff.data_ptr(), dlen.data_ptr(), scratch.data_ptr(),
                                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:start] == CANARY).all() and (got[start + capacity:] == CANARY).all()
    assert np.array_equal(dsrc.cpu().numpy().reshape(-1)[:src.size], np.ascontiguousarray(src).reshape(-1))
    return rc, dlen.cpu().numpy()[:slots], doff.cpu().numpy(), got[start:start + capacity]


def check_case(sh, B, groups, emax, blocks, count, misalign=0, stride=None, src_skip=0, capacity=None):
    stride = emax if stride is None else stride
    flat = blocks.reshape(-1)
    want_len, want_off, _, _ = unframe_rule(B, groups, emax, stride, flat[src_skip:], count, None)
    total = int(want_off[-1])
    capacity = total if capacity is None else capacity
    want_len, want_off, want_pay, errors = unframe_rule(B, groups, emax, stride, flat[src_skip:], count, capacity)
    rc, got_len, got_off, got_pay = run_unframe(sh, B, groups, emax, stride, blocks, count, capacity,
                                                misalign=misalign, src_skip=src_skip)
    assert rc == 0
    assert np.array_equal(got_len, want_len), np.flatnonzero(got_len != want_len)[:8]
    assert np.array_equal(got_off, want_off), np.flatnonzero(got_off != want_off)[:8]
    assert np.array_equal(got_pay, want_pay), np.flatnonzero(got_pay != want_pay)[:8]
    return errors, want_len, want_off


# ---------------------------------------------------------------- CPU

def test_unframe_symbols_exported():
    import shorthair_amd as sh
    from shorthair_amd import groups as sg
    for name in ("shorthair_unframe_batch", "shorthair_unframe_scratch_bytes", "shorthair_groups_set_delivery"):
        assert name in sh.EXPORTED_SYMBOLS
        assert getattr(sh.lib, name) is not None
    assert callable(sh.unframe_batch) and callable(sh.unframe_scratch_bytes) and callable(sg.set_delivery)


def test_unframe_rejects_bad_arguments_without_gpu():
    """Every host-checked argument returns -1 before anything touches the GPU (there is none here)."""
    import shorthair_amd as sh
    f = sh.lib.shorthair_unframe_batch
    p = 0x1000  # never dereferenced

    def call(B=16, groups=4, emax=2, stride=2, out=p, count=None, pay=p, cap=64, off=p, ln=p, scr=p):
        return f(B, groups, emax, stride, out, count, pay, cap, off, ln, scr, None)

    assert call(B=0) == -1            # block_bytes < 8
    assert call(B=4) == -1
    assert call(B=-8) == -1
    assert call(B=12) == -1           # block_bytes % 8
    assert call(B=1353) == -1
    assert call(groups=-1) == -1      # groups < 0
    assert call(emax=0) == -1         # emax outside 1..255
    assert call(emax=-1) == -1
    assert call(emax=256, stride=256) == -1
    assert call(groups=INT_MAX // 255 + 1, emax=255, stride=255) == -1  # groups * emax > INT_MAX
    assert call(groups=INT_MAX, emax=2) == -1
    assert call(stride=1) == -1       # group_stride_blocks < emax
    assert call(stride=-5) == -1
    assert call(cap=-1) == -1         # payload_capacity < 0
    for mis in (1, 2, 4, 7, 12):      # d_out not 8-byte aligned
        assert call(out=p + mis) == -1
        assert call(groups=0, out=p + mis) == -1
    for mis in (1, 2, 4, 7, 12):      # d_off not 8-byte aligned
        assert call(off=p + mis) == -1
    for mis in (1, 2, 3, 6):          # d_len not 4-byte aligned
        assert call(ln=p + mis) == -1
    assert call(out=None) == -1       # null pointers with groups > 0
    assert call(off=None) == -1
    assert call(ln=None) == -1
    assert call(scr=None) == -1
    assert call(pay=None) == -1       # null d_payload with payload_capacity > 0
    assert call(groups=0) == 0        # an empty batch is fine, and no GPU work
    assert f(16, 0, 1, 1, None, None, None, 0, None, None, None, None) == 0


def test_unframe_scratch_bytes():
    import shorthair_amd as sh
    f = sh.lib.shorthair_unframe_scratch_bytes
    for groups, emax in ((-1, 1), (1, 0), (1, -1), (1, 256), (INT_MAX, 2), (INT_MAX // 255 + 1, 255)):
        assert f(groups, emax) == -1
        with pytest.raises(ValueError):
            sh.unframe_scratch_bytes(groups, emax)
    assert f(0, 1) > 0 and f(INT_MAX, 1) > 0 and f(INT_MAX // 255, 255) > 0
    for emax in (1, 5, 32, 255):
        sizes = [f(g, emax) for g in (0, 1, 2, 51, 52, 256, 257, 70001, 1 << 20)]
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes)
    for groups in (1, 40, 8192):
        sizes = [f(groups, e) for e in range(1, 256)]
        assert sizes == sorted(sizes)
    assert sh.unframe_scratch_bytes(8192, 32) == f(8192, 32)


def test_unframe_scratch_bytes_needs_no_gpu():
    """A fresh process: the size comes back without a GPU (there is none here), and nothing fails."""
    code = ("import shorthair_amd as sh; n = sh.lib.shorthair_unframe_scratch_bytes(8192, 32); "
            "assert n > 0; assert sh.lib.shorthair_unframe_scratch_bytes(8192, 0) == -1; print('ok', n)")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-800:]
    assert "libcauchy256" not in r.stderr  # no GPU/runtime failure message: the GPU was never asked for


def test_rule_restatement_matches_oracle_rx_group():
    """The numpy rule above delivers exactly what oracle/packets.py's rx_group does: a group decoded
    by the oracle, its recovered blocks laid out as d_out with stale slots behind them."""
    ora = po.oracle()
    rng = np.random.default_rng(4)
    B, m = 16, 4
    packets = [rng.integers(0, 256, size=n, dtype=np.uint8).tobytes() for n in (0, 1, 5, 6, 7, 13, 14, 9)]
    k = len(packets)
    rec = opk.tx_group(ora, m, packets)
    lost = [1, 4, 6]
    orig = [(i, packets[i]) for i in (7, 0, 3, 2, 5)]
    got = [rec[2], rec[0], rec[3]]
    want = opk.rx_group(ora, orig, got)
    assert [pid for pid, _ in want] == lost and [p for _, p in want] == [packets[i] for i in lost]
    # the decode rx_group makes, kept: blocks n_orig..k-1 are the recovered originals
    datas, rows = [], []
    for oid, p in orig:
        b = np.zeros(B, np.uint8)
        put_prefix(b[None], 0, len(p))
        b[2:2 + len(p)] = np.frombuffer(p, np.uint8)
        datas.append(b)
        rows.append(oid)
    for r in got:
        datas.append(np.frombuffer(r[3:], np.uint8).copy())
        rows.append(r[0])
    rc, new_rows = ora.decode(k, m, datas, rows, B)
    assert rc == 0
    emax, e = min(k, m), len(lost)
    d_out = rng.integers(0, 256, size=(emax, B), dtype=np.uint8)  # stale behind the count
    put_prefix(d_out, emax - 1, 3)
    for i in range(e):
        d_out[i] = datas[len(orig) + i]
    length, off, pay, errors = unframe_rule(B, 1, emax, emax, d_out.reshape(-1), np.array([e]), 1 << 12)
    delivered = [(int(new_rows[len(orig) + i]), pay[off[i]:off[i] + length[i]].tobytes())
                 for i in range(emax) if length[i] >= 0]
    assert delivered == want and errors == 0
    assert list(length[e:]) == [-1] * (emax - e) and off[emax] == sum(len(p) for _, p in want)


# ---------------------------------------------------------------- GPU: kernel against the rule

SHAPES = [(1, 1), (63, 1), (257, 1), (13, 5), (52, 5), (40, 32)]  # slots 1, 63, 257, 65, 260, 1280


@pytest.mark.gpu
@pytest.mark.parametrize("B", [8, 16, 24, 136, 1352])
def test_unframe_matches_rule(sh, B):
    assert SHAPES[-1][0] * SHAPES[-1][1] > 4 * sh.UNFRAME_TILE_SLOTS  # several tiles
    sh.batch_errors()
    for groups, emax in SHAPES:
        for misalign in (0, 1, 3, 8, 13):
            blocks, count = build_case(B, groups, emax, seed=B * 100000 + groups * 100 + emax * 16 + misalign)
            errors, want_len, _ = check_case(sh, B, groups, emax, blocks, count, misalign=misalign)
            assert errors == 0
            assert (want_len >= 0).sum() == int(count.sum())
    assert sh.batch_errors() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("B", [8, 16])
def test_unframe_many_tiles(sh, B):
    """70,001 slots: more tile sums than one pass of the scan workgroup takes."""
    groups, emax = 70001, 1
    tiles = -(-groups * emax // sh.UNFRAME_TILE_SLOTS)
    assert tiles > sh.UNFRAME_SCAN_PASS
    sh.batch_errors()
    blocks, count = build_case(B, groups, emax, seed=B)
    errors, _, want_off = check_case(sh, B, groups, emax, blocks, count, misalign=3)
    assert errors == 0 and want_off[-1] > 0
    assert sh.batch_errors() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("k", [2, 7])
def test_unframe_strided_m1_form(sh, k):
    """The in-place m = 1 decode: the recovered block is block k - 1 of each group of [groups][k][B]."""
    sh.batch_errors()
    for B, groups in ((24, 70), (136, 300)):
        blocks, _ = build_case(B, groups, 1, seed=k * 1000 + B, stride=k, with_count=False)
        # build_case put the prefixes on block 0 of each group: the case wants them on block k - 1
        blocks = np.ascontiguousarray(np.roll(blocks, k - 1, axis=0))
        errors, want_len, _ = check_case(sh, B, groups, 1, blocks, None, misalign=1, stride=k, src_skip=(k - 1) * B)
        assert errors == 0 and (want_len >= 0).all()
    assert sh.batch_errors() == 0


@pytest.mark.gpu
def test_unframe_malformed_and_dropped(sh):
    """One of each among good slots: prefixes B - 1 and 65535 (dropped, d_len = -2, no error), a group
    flagged -1 by the decode (nothing, no error), counts -2 and emax + 1 (nothing, one error each)."""
    B, groups, emax = 136, 12, 5
    blocks, count = build_case(B, groups, emax, seed=31)
    count[:] = emax
    count[3], count[6], count[9] = -1, -2, emax + 1
    put_prefix(blocks, 1 * emax + 2, B - 1)
    put_prefix(blocks, 7 * emax + 0, 65535)
    sh.batch_errors()
    errors, want_len, want_off = check_case(sh, B, groups, emax, blocks, count, misalign=13)
    assert errors == 2
    assert sh.batch_errors() == 2
    assert sh.batch_errors() == 0
    assert want_len[1 * emax + 2] == -2 and want_len[7 * emax] == -2
    for g in (3, 6, 9):
        assert (want_len[g * emax:(g + 1) * emax] == -1).all()
    assert (want_len >= 0).sum() == (groups - 3) * emax - 2


@pytest.mark.gpu
def test_unframe_capacity(sh):
    B, groups, emax = 136, 9, 5
    blocks, count = build_case(B, groups, emax, seed=41)
    count[-1] = emax
    put_prefix(blocks, groups * emax - 1, 77)  # the last slot delivers a non-empty payload
    flat = blocks.reshape(-1)
    want_len, want_off, _, _ = unframe_rule(B, groups, emax, emax, flat, count, None)
    total = int(want_off[-1])
    sh.batch_errors()
    # one byte short: the last payload is not written at all and counted once
    errors, _, off1 = check_case(sh, B, groups, emax, blocks, count, misalign=3, capacity=total - 1)
    assert errors == 1 and off1[-1] == total
    assert sh.batch_errors() == 1
    # nothing fits, and there is no buffer: every non-empty payload is counted, nothing faults
    nonempty = int((want_len > 0).sum())
    assert 0 < nonempty < (want_len >= 0).sum()  # an empty payload has an empty span: never counted
    rc, got_len, got_off, _ = run_unframe(sh, B, groups, emax, emax, blocks, count, 0, null_payload=True)
    assert rc == 0 and np.array_equal(got_len, want_len) and np.array_equal(got_off, want_off)
    assert got_off[-1] == total
    assert sh.batch_errors() == nonempty


@pytest.mark.gpu
def test_unframe_length_limit_of_a_long_block(sh):
    """B - 2 > 65535: every u16 prefix delivers, 65535 included (65536 cannot occur)."""
    B, groups, emax = 65544, 2, 2
    blocks, _ = build_case(B, groups, emax, seed=5, with_count=False)
    for j, p in enumerate((65535, 9, 0, 65535)):
        put_prefix(blocks, j, p)
    sh.batch_errors()
    errors, want_len, want_off = check_case(sh, B, groups, emax, blocks, None, misalign=1)
    assert list(want_len) == [65535, 9, 0, 65535] and want_off[-1] == 2 * 65535 + 9
    assert errors == 0 and sh.batch_errors() == 0


@pytest.mark.gpu
def test_unframe_then_frame_round_trip(sh):
    """(d_payload, d_off, d_len) of the delivered slots is valid input for frame_batch: it rebuilds
    bytes [0, 2 + p) of each source block and zeros behind them."""
    import torch
    B, groups, emax = 136, 21, 5
    blocks, count = build_case(B, groups, emax, seed=61)
    put_prefix(blocks, 4, B - 1)  # a dropped block in a full group
    slots = groups * emax
    flat = blocks.reshape(-1)
    want_len, want_off, _, _ = unframe_rule(B, groups, emax, emax, flat, count, None)
    total = int(want_off[-1])
    pay = torch.zeros(total, dtype=torch.uint8, device="cuda")
    doff = torch.zeros(slots + 1, dtype=torch.int64, device="cuda")
    dlen = torch.zeros(slots, dtype=torch.int32, device="cuda")
    scratch = torch.zeros(sh.unframe_scratch_bytes(groups, emax), dtype=torch.uint8, device="cuda")
    sh.batch_errors()
    assert sh.unframe_batch(B, groups, emax, emax, _dev(blocks), _dev(count), pay, total, doff, dlen, scratch) == 0
    keep = torch.nonzero(dlen >= 0).flatten()
    n = int(keep.numel())
    assert n == (want_len >= 0).sum() > 0
    back = torch.full((n, B), 0x5A, dtype=torch.uint8, device="cuda")
    assert sh.frame_batch(B, n, pay, total, doff[:-1][keep].contiguous(), dlen[keep].contiguous(), None, back) == 0
    assert sh.batch_errors() == 0
    back = back.cpu().numpy()
    for j, s in enumerate(np.flatnonzero(want_len >= 0)):
        p = int(want_len[s])
        assert np.array_equal(back[j, :2 + p], blocks[s, :2 + p]) and not back[j, 2 + p:].any(), s


@pytest.mark.gpu
def test_unframe_python_binding_on_tensors(sh):
    import torch
    B, groups, emax = 24, 63, 5
    blocks, count = build_case(B, groups, emax, seed=71)
    slots = groups * emax
    want_len, want_off, want_pay, _ = unframe_rule(B, groups, emax, emax, blocks.reshape(-1), count, 4096 * 4)
    pay = torch.full((4096 * 4,), CANARY, dtype=torch.uint8, device="cuda")
    doff = torch.zeros(slots + 1, dtype=torch.int64, device="cuda")
    dlen = torch.zeros(slots, dtype=torch.int32, device="cuda")
    scratch = torch.zeros(sh.unframe_scratch_bytes(groups, emax), dtype=torch.uint8, device="cuda")
    assert sh.unframe_batch(B, groups, emax, emax, _dev(blocks), _dev(count), pay, pay.numel(), doff, dlen,
                            scratch) == 0
    torch.cuda.synchronize()
    assert np.array_equal(dlen.cpu().numpy(), want_len) and np.array_equal(doff.cpu().numpy(), want_off)
    assert np.array_equal(pay.cpu().numpy(), want_pay)


# ---------------------------------------------------------------- GPU: composition with the codec calls

COMPOSE = [(28, 4, 136, "fixed"), (20, 10, 136, "tile"), (20, 5, 24, "generic")]
GAP = 0xA5


@functools.lru_cache(maxsize=None)
def compose_case(kmax, m, B):
    """Groups of payloads, their oracle recovery packets, and one receive pattern per group with the
    oracle's deliveries."""
    ora = po.oracle()
    rng = np.random.default_rng(kmax * 100 + m + 1)
    ks = [kmax, 2] + [int(v) for v in rng.integers(max(2, (6 * kmax + 9) // 10), kmax + 1, size=4)]
    rx, want = [], []
    for k in ks:
        lens = [int(v) for v in rng.integers(0, B - 1, size=k)]
        lens[int(rng.integers(0, k))] = B - 2  # the group's largest payload sets block_bytes
        pk = [rng.integers(0, 256, size=n, dtype=np.uint8).tobytes() for n in lens]
        rec = opk.tx_group(ora, m, pk)
        assert len(rec[0]) == 3 + B
        e = int(rng.integers(1, min(k, m) + 1))
        lost = set(int(x) for x in rng.choice(k, size=e, replace=False))
        orig = [(i, pk[i]) for i in range(k) if i not in lost]
        orig = [orig[i] for i in rng.permutation(len(orig))]
        got = [rec[int(y)] for y in rng.choice(m, size=e, replace=False)]
        rx.append((orig, got))
        want.append(opk.rx_group(ora, orig, got))
    return ks, rx, want


@pytest.mark.gpu
@pytest.mark.parametrize("shape", COMPOSE, ids=lambda s: "k%d_m%d_B%d_%s" % s)
def test_frame_decode_unframe_matches_oracle_packets(sh, shape):
    """frame_batch -> decode_batch_out_var -> unframe_batch, all on device arrays: the delivered
    (out_rows[s], payload) lists per group are rx_group's."""
    import torch
    kmax, m, B, family = shape
    assert sh.path(kmax, m, B) == family
    ks, rx, want = compose_case(kmax, m, B)
    G = len(ks)
    rng = np.random.default_rng(10)
    first = np.concatenate([[0], np.cumsum(ks)]).astype(np.int32)
    total = int(first[-1])
    parts, off, length, raw, rows, pos = [], [], [], [], [], 0
    for orig, pkts in rx:
        for data, skip, ln, r, row in [(p, 0, len(p), 0, oid) for oid, p in orig] + \
                                      [(pkt, 3, B, 1, pkt[0]) for pkt in pkts]:
            gap = int(rng.integers(0, 7))
            parts += [np.full(gap, GAP, np.uint8), np.frombuffer(data, np.uint8)]
            off.append(pos + gap + skip)
            pos += gap + len(data)
            length.append(ln)
            raw.append(r)
            rows.append(row)
    payload = np.concatenate(parts)
    sh.batch_errors()
    blocks = torch.zeros((total, B), dtype=torch.uint8, device="cuda")
    assert sh.frame_batch(B, total, _dev(payload), len(payload), _dev(np.array(off, np.int64)),
                          _dev(np.array(length, np.int32)), _dev(np.array(raw, np.uint8)), blocks) == 0
    emax = min(kmax, m)
    slots = G * emax
    out = torch.full((G, emax, B), 0x77, dtype=torch.uint8, device="cuda")  # stale behind each count
    out_rows = torch.zeros((G, emax), dtype=torch.uint8, device="cuda")
    count = torch.full((G,), -7, dtype=torch.int32, device="cuda")
    assert sh.decode_batch_out_var(kmax, m, B, G, _dev(first), total, blocks, _dev(np.array(rows, np.uint8)), out,
                                   out_rows, count) == 0
    cap = slots * (B - 2)
    pay = torch.full((cap,), CANARY, dtype=torch.uint8, device="cuda")
    doff = torch.zeros(slots + 1, dtype=torch.int64, device="cuda")
    dlen = torch.zeros(slots, dtype=torch.int32, device="cuda")
    scratch = torch.zeros(sh.unframe_scratch_bytes(G, emax), dtype=torch.uint8, device="cuda")
    assert sh.unframe_batch(B, G, emax, emax, out, count, pay, cap, doff, dlen, scratch) == 0
    assert sh.batch_errors() == 0
    pay, doff, dlen = pay.cpu().numpy(), doff.cpu().numpy(), dlen.cpu().numpy()
    out_rows = out_rows.cpu().numpy()
    for g in range(G):
        delivered = [(int(out_rows[g, i]), pay[doff[s]:doff[s] + dlen[s]].tobytes())
                     for i in range(emax) for s in [g * emax + i] if dlen[s] >= 0]
        assert delivered == want[g], g
    assert doff[slots] == sum(len(p) for w in want for _, p in w)
    assert (pay[doff[slots]:] == CANARY).all()
