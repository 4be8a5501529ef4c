"""Device-resident listing of received packets (include/shorthair_rx.h: shorthair_rx_list_batch).

Expected values come from the rule of the header restated in numpy below (rx_list_rule) and, for the
decodes, from oracle/packets.py on the CPU oracle -- never from the library under test.
"""
import os

import numpy as np
import pytest

from oracle import packets as opk
from oracle import pyoracle as po
from tests.test_frame import COMPOSE, GAP, _pack, compose_case, frame_rule

CANARY = 0xC3
PAD = 1024
MAXP = 512      # SHORTHAIR_RX_MAX_PACKETS
INFO = 8        # SHORTHAIR_RX_INFO_INTS
SCAN_TILE = 16  # SHORTHAIR_RX_SCAN_TILE
SCAN_PASS = 4096  # SHORTHAIR_RX_SCAN_PASS
BAD = ((-1, 0, 0, 0, 0, 0, -1), [])


# ---------------------------------------------------------------- the rule

def rx_group_rule(kmin, kmax, m_arg, B_arg, packets, ring, pkt_first, pkt_off, pkt_len, g):
    """Steps 0 to 8 for group g: ((status, k, m, B, n_orig, n_rec, first_rec), [(off, len, raw, row)])."""
    f0, f1 = int(pkt_first[g]), int(pkt_first[g + 1])
    if f0 < 0 or f1 < f0 or f1 > packets or f1 - f0 > MAXP:
        return BAD
    recs = []
    for p in range(f0, f1):
        off, ln = int(pkt_off[p]), int(pkt_len[p])
        if ln < 2 or off < 0 or off + ln > len(ring):
            return BAD
        recs.append((p, off, ln, int(ring[off]), int(ring[off + 1])))
    orig = [r for r in recs if r[3] <= r[4]]
    rec = [r for r in recs if r[3] > r[4]]
    n_orig, n_rec = len(orig), len(rec)
    if not rec:
        return (0, 0, 0, 0, n_orig, 0, -1), []
    first_rec, k = rec[0][0], rec[0][4] + 1
    if any(r[4] + 1 != k for r in rec):
        return BAD
    if k == 1:
        return (2 if n_orig == 0 else 0, 1, 0, 0, n_orig, n_rec, first_rec), []
    if n_orig >= k or n_orig + n_rec < k:
        return (0, k, 0, 0, n_orig, n_rec, first_rec), []
    _, off, ln, _, _ = rec[-1]
    if ln < 3:
        return BAD
    m, B = int(ring[off + 2]) + 1, ln - 3
    if B < 8 or B % 8 != 0 or k + m > 256:
        return BAD
    seen = set()
    for _, off, ln, rid, c in orig:
        if c >= k or rid in seen or ln - 2 > B - 2:
            return BAD
        seen.add(rid)
    use = k - n_orig
    for _, off, ln, rid, c in rec[:use]:
        if not k <= rid < k + m or rid in seen or ln != B + 3:
            return BAD
        seen.add(rid)
    status = 1 if kmin <= k <= kmax and m == m_arg and B == B_arg else 3
    blocks = [(off + 2, ln - 2, 0, rid) for _, off, ln, rid, _ in orig]
    blocks += [(off + 3, B, 1, rid) for _, off, ln, rid, _ in rec[:use]]
    return (status, k, m, B, n_orig, n_rec, first_rec), blocks


def rx_list_rule(kmin, kmax, m, B, groups, packets, pkt_first, pkt_off, pkt_len, ring):
    """Every output of shorthair_rx_list_batch by the rule of shorthair_rx.h, as a dict of arrays."""
    cap = min(packets, groups * kmax)
    info = np.zeros((groups, INFO), np.int32)
    first = np.zeros(groups + 1, np.int32)
    slot_group = np.full(groups, -1, np.int32)
    off, ln = np.zeros(cap, np.int64), np.zeros(cap, np.int32)
    raw, rows = np.zeros(cap, np.uint8), np.zeros(cap, np.uint8)
    n_listed = total = 0
    prefix = 0  # blocks of the groups step 8 listed
    for g in range(groups):
        (status, k, gm, gB, n_orig, n_rec, first_rec), blocks = rx_group_rule(
            kmin, kmax, m, B, packets, ring, pkt_first, pkt_off, pkt_len, g)
        slot = -1
        if status == 1:
            if prefix + k <= cap:
                slot = n_listed
                slot_group[slot] = g
                for j, (o, l, r, row) in enumerate(blocks):
                    off[total + j], ln[total + j], raw[total + j], rows[total + j] = o, l, r, row
                total += k
                n_listed += 1
                first[n_listed] = total
            else:  # step 9
                (status, k, gm, gB, n_orig, n_rec, first_rec), _ = BAD
            prefix += len(blocks)
        info[g] = (status, k, gm, gB, n_orig, n_rec, slot, first_rec)
    first[n_listed + 1:] = total
    st = info[:, 0]
    summary = np.array([n_listed, total, (st == 0).sum(), (st == 2).sum(), (st == 3).sum(), (st == -1).sum(), 0, 0],
                       np.int32)
    return dict(info=info, first=first, slot_group=slot_group, off=off, len=ln, raw=raw, rows=rows, summary=summary)


# ---------------------------------------------------------------- building batches

def orig_rec(rid, payload, c=None):
    return bytes([rid, rid if c is None else c]) + bytes(payload)


def recov_rec(rid, k, m, block):
    return bytes([rid, k - 1, m - 1]) + bytes(block)


def merge(rng, a, b):
    """A random interleaving of the two lists that keeps the order inside each."""
    pick = np.zeros(len(a) + len(b), bool)
    pick[rng.choice(len(pick), size=len(a), replace=False)] = True
    ia, ib = iter(a), iter(b)
    return [next(ia) if t else next(ib) for t in pick]


def sized_group(rng, k, m, B, n):
    """n records of a (k, m, B) group in arrival order: decodable whenever n >= k; recovery records past
    the ones the decode uses carry repeated ids and odd lengths, the last one the group's m and B."""
    def body(ln):
        return rng.integers(0, 256, size=ln, dtype=np.uint8).tobytes()
    if n >= k:
        n_orig = int(rng.integers(max(0, k - m), k))
    else:
        n_orig = n // 2
    n_rec = n - n_orig
    ids = [int(v) for v in rng.permutation(k)[:n_orig]]
    orig = [orig_rec(i, body(int(rng.integers(0, B - 1))), c=int(rng.integers(i, k)) if rng.integers(0, 4) == 0 else None)
            for i in ids]
    use = max(min(k - n_orig, n_rec, m), 0)
    rec = [recov_rec(k + int(y), k, m, body(B)) for y in rng.permutation(m)[:use]]
    for j in range(use, n_rec):
        rid = int(rng.integers(k, 256))
        if j == n_rec - 1:
            rec.append(recov_rec(rid, k, m, body(B)))
        else:
            rec.append(bytes([rid, k - 1]) + body(int(rng.choice([0, 1, B + 1, 3]))))
    return merge(rng, orig, rec)


def lay_out(rng, groups, scatter=True):
    """groups: [[record bytes]] -> (ring, pkt_first, pkt_off, pkt_len). The records lie in the ring in a
    shuffled order with gaps of 0..7 GAP bytes, so that their offsets take every value mod 8; the last
    one ends exactly at ring_bytes."""
    recs = [r for grp in groups for r in grp]
    pkt_first = np.concatenate([[0], np.cumsum([len(grp) for grp in groups])]).astype(np.int32)
    order = rng.permutation(len(recs)) if scatter else np.arange(len(recs))
    pkt_off = np.zeros(len(recs), np.int64)
    parts, pos = [], 0
    for j, p in enumerate(order):
        gap = j % 8 if j < 16 else int(rng.integers(0, 8))
        gap = (gap - pos) % 8 if j < 16 else gap  # the first 16 records: offset = j (mod 8)
        parts.append(np.full(gap, GAP, np.uint8))
        pos += gap
        pkt_off[p] = pos
        parts.append(np.frombuffer(recs[p], np.uint8))
        pos += len(recs[p])
    ring = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    pkt_len = np.array([len(r) for r in recs], np.int32)
    return ring, pkt_first, pkt_off, pkt_len


# ---------------------------------------------------------------- running on the GPU

@pytest.fixture(scope="module")
def sh():
    import torch
    import shorthair_amd
    assert shorthair_amd.cauchy_256_init() == 0
    torch.cuda.init()
    return shorthair_amd


class Guarded:
    """`nbytes` of device memory between canaries at an address = mis (mod 16)."""

    def __init__(self, nbytes, mis, data=None):
        import torch
        self.n = nbytes
        self.buf = torch.full((PAD + 16 + nbytes + PAD,), CANARY, dtype=torch.uint8, device="cuda")
        self.start = PAD + (mis - (self.buf.data_ptr() + PAD)) % 16
        self.ptr = self.buf.data_ptr() + self.start
        assert self.ptr % 16 == mis
        self.data = None
        if data is not None:
            self.data = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
            assert len(self.data) == nbytes
            if nbytes:
                self.buf[self.start:self.start + nbytes] = torch.from_numpy(self.data.copy()).cuda()

    def tensor(self, dtype):
        """The guarded bytes as a tensor of `dtype` (a view: what the Python binding takes)."""
        return self.buf[self.start:self.start + self.n].view(dtype)

    def read(self, dtype):
        got = self.buf.cpu().numpy()
        assert (got[:self.start] == CANARY).all() and (got[self.start + self.n:] == CANARY).all(), "canary"
        return got[self.start:self.start + self.n].copy().view(dtype)

    def unchanged(self):
        return np.array_equal(self.read(np.uint8), self.data)


def guarded_outputs(groups, cap, variant):
    """Every output array of the call between canaries, as {name: (Guarded, dtype)}. Variant 0: bases of
    the least alignment the contract allows (4 for ints, 8 for d_off, odd for bytes); 1: 16-byte aligned."""
    lo = variant == 0
    i4, i8 = (4, 8) if lo else (0, 0)
    return dict(info=(Guarded(4 * INFO * groups, i4), np.int32), first=(Guarded(4 * (groups + 1), i4 + 8 * lo), np.int32),
                slot_group=(Guarded(4 * groups, i4), np.int32), off=(Guarded(8 * cap, i8), np.int64),
                len=(Guarded(4 * cap, i4 + 8 * lo), np.int32), raw=(Guarded(cap, 3 if lo else 0), np.uint8),
                rows=(Guarded(cap, 7 if lo else 0), np.uint8), summary=(Guarded(32, i4), np.int32))


def run_rx(sh, kmin, kmax, m, B, groups, packets, pkt_first, pkt_off, pkt_len, ring, variant=0, ring_bytes=None):
    """Runs the call with every array between canaries at the bases of alignment variant `variant` (0: the
    least the contract allows -- 4 for ints, 8 for 64-bit arrays and the scratch, odd for bytes; 1: 16),
    checks the canaries and that the inputs are unchanged, and returns (rc, outputs as rx_list_rule's)."""
    import torch
    lo = variant == 0
    i4, i8 = (4, 8) if lo else (0, 0)
    cap = sh.rx_list_capacity(groups, packets, kmax)
    ring_bytes = len(ring) if ring_bytes is None else ring_bytes
    d_first_in = Guarded(4 * (groups + 1), i4 + 8 * lo, np.asarray(pkt_first, np.int32))
    d_off_in = Guarded(8 * packets, i8, np.asarray(pkt_off, np.int64))
    d_len_in = Guarded(4 * packets, i4, np.asarray(pkt_len, np.int32))
    d_ring = Guarded(len(ring), 5 if lo else 0, ring)
    out = guarded_outputs(groups, cap, variant)
    scratch = Guarded(sh.rx_list_scratch_bytes(groups, packets), i8)
    p = {name: gd.ptr for name, (gd, _) in out.items()}
    rc = sh.lib.shorthair_rx_list_batch(kmin, kmax, m, B, groups, packets, d_first_in.ptr, d_off_in.ptr, d_len_in.ptr,
                                        d_ring.ptr, ring_bytes, p["info"], p["first"], p["slot_group"], p["off"],
                                        p["len"], p["raw"], p["rows"], p["summary"], scratch.ptr,
                                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    scratch.read(np.uint8)  # canaries
    assert d_first_in.unchanged() and d_off_in.unchanged() and d_len_in.unchanged() and d_ring.unchanged()
    got = {name: gd.read(dt) for name, (gd, dt) in out.items()}
    got["info"] = got["info"].reshape(groups, INFO)
    return rc, got


def assert_same(got, want, tag):
    for name in ("summary", "info", "first", "slot_group", "off", "len", "raw", "rows"):
        assert got[name].shape == want[name].shape, (tag, name)
        if not want[name].size:
            continue
        bad = np.flatnonzero((got[name] != want[name]).reshape(len(want[name]), -1).any(axis=1))
        assert not len(bad), (tag, name, bad[:6], got[name][bad[:3]], want[name][bad[:3]])


# ---------------------------------------------------------------- CPU

def test_rx_symbols_exported():
    import shorthair_amd as sh
    for name in ("shorthair_rx_list_batch", "shorthair_rx_list_capacity", "shorthair_rx_list_scratch_bytes"):
        assert name in sh.EXPORTED_SYMBOLS
        assert getattr(sh.lib, name) is not None
    assert callable(sh.rx_list_batch) and callable(sh.rx_list_capacity) and callable(sh.rx_list_scratch_bytes)
    assert (sh.RX_MAX_PACKETS, sh.RX_INFO_INTS, sh.RX_SCAN_TILE, sh.RX_SCAN_PASS) == (MAXP, INFO, SCAN_TILE, SCAN_PASS)
    text = open(os.path.join(os.path.dirname(__file__), "..", "include", "shorthair_rx.h")).read()
    for name, value in (("MAX_PACKETS", MAXP), ("INFO_INTS", INFO), ("SCAN_TILE", SCAN_TILE), ("SCAN_PASS", SCAN_PASS)):
        assert "#define SHORTHAIR_RX_%s %d " % (name, value) in text, name


def test_rx_rejects_bad_arguments_without_gpu(capfd):
    """Every host-checked argument returns -1 before anything touches the GPU (there is none here: an
    initialisation attempt would print the library's "no HIP device" error)."""
    import shorthair_amd as sh
    f = sh.lib.shorthair_rx_list_batch
    p = 0x1000  # never dereferenced
    names = ["pkt_first", "pkt_off", "pkt_len", "ring", "info", "first", "slot_group", "off", "len", "raw", "rows",
             "summary", "scratch"]

    def call(kmin=2, kmax=20, m=4, B=16, groups=4, packets=40, ring_bytes=4096, **ptrs):
        a = {n: p for n in names}
        a.update(ptrs)
        return f(kmin, kmax, m, B, groups, packets, a["pkt_first"], a["pkt_off"], a["pkt_len"], a["ring"], ring_bytes,
                 a["info"], a["first"], a["slot_group"], a["off"], a["len"], a["raw"], a["rows"], a["summary"],
                 a["scratch"], None)

    assert call(groups=0) == 0                                    # an empty batch is fine, and no GPU work
    assert call(groups=0, packets=0, **{n: None for n in names}) == 0
    for kmin, kmax in ((1, 20), (0, 20), (-1, 20), (21, 20), (2, 256), (2, 300), (256, 256)):
        assert call(kmin=kmin, kmax=kmax, m=1) == -1, (kmin, kmax)   # 2 <= kmin <= kmax <= 255
    for m in (0, -1):
        assert call(m=m) == -1                                    # m >= 1
    assert call(kmax=200, m=57) == -1 and call(kmax=255, m=2) == -1  # kmax + m <= 256
    for B in (0, 4, -8, 12, 1353):
        assert call(B=B) == -1                                    # block_bytes >= 8, a multiple of 8
    assert call(groups=-1) == -1 and call(packets=-1) == -1 and call(ring_bytes=-1) == -1
    for n in ("pkt_first", "pkt_len", "info", "first", "slot_group", "len", "summary"):
        for mis in (1, 2, 3):                                     # 4-byte alignment of the int arrays
            assert call(**{n: p + mis}) == -1, (n, mis)
            assert call(groups=0, **{n: p + mis}) == -1, (n, mis)
        assert call(groups=0, **{n: p + 4}) == 0
    for n in ("pkt_off", "off", "scratch"):
        for mis in (1, 2, 4, 7, 12):                              # 8-byte alignment
            assert call(**{n: p + mis}) == -1, (n, mis)
            assert call(groups=0, **{n: p + mis}) == -1, (n, mis)
        assert call(groups=0, **{n: p + 8}) == 0
    for n in names:                                               # null pointers with groups > 0
        assert call(**{n: None}) == -1, n
    assert call(packets=0, pkt_off=None, pkt_len=None, ring=None, off=None, len=None, raw=None, rows=None,
                info=None) == -1                                  # (the rest may be null at packets == 0: not info)
    assert call(groups=0, raw=p + 1, rows=p + 3, ring=p + 5) == 0  # byte arrays take any address

    cap, scr = sh.lib.shorthair_rx_list_capacity, sh.lib.shorthair_rx_list_scratch_bytes
    assert cap(4, 100, 20) == 80 and cap(4, 50, 20) == 50 and cap(0, 50, 20) == 0 and cap(4, 0, 20) == 0
    assert cap(2**31 - 1, 2**31 - 1, 255) == 2**31 - 1
    for bad in ((-1, 10, 20), (4, -1, 20), (4, 10, 1), (4, 10, 256), (4, 10, 0)):
        assert cap(*bad) == -1, bad
    assert scr(-1, 0) == -1 and scr(0, -1) == -1
    sizes = [[scr(g, n) for n in (0, 1, 2, 3, 4, 5, 100, 4097, 2**31 - 1)] for g in (0, 1, 2, 17, 4097, 2**31 - 1)]
    assert all(v > 0 for row in sizes for v in row)
    assert all(a <= b for row in sizes for a, b in zip(row, row[1:]))
    assert all(a <= b for r0, r1 in zip(sizes, sizes[1:]) for a, b in zip(r0, r1))
    with pytest.raises(ValueError):
        sh.rx_list_capacity(4, 10, 1)
    with pytest.raises(ValueError):
        sh.rx_list_scratch_bytes(-1, 0)
    assert "libcauchy256" not in capfd.readouterr().err


def deliveries(ora, B, ring, res, slot):
    """What RecoverGroup delivers for a listed slot: the listed blocks framed by frame_rule, decoded on
    the CPU oracle, cut by the length prefix (oracle/packets.py rx_group, :741-756)."""
    g = int(res["slot_group"][slot])
    _, k, m, gB, n_orig = (int(v) for v in res["info"][g][:5])
    assert gB == B
    f0, f1 = int(res["first"][slot]), int(res["first"][slot + 1])
    assert f1 - f0 == k
    blocks = frame_rule(B, ring, res["off"][f0:f1], res["len"][f0:f1], res["raw"][f0:f1])
    assert all(b.any() or res["len"][f0 + j] == 0 for j, b in enumerate(blocks))
    datas = [b.copy() for b in blocks]
    rows = [int(r) for r in res["rows"][f0:f1]]
    rc, new_rows = ora.decode(k, m, datas, rows, B)
    assert rc == 0
    missing = sorted(set(range(k)) - set(rows[:n_orig]))
    out = []
    for ii in range(n_orig, k):
        ln = int(datas[ii][0]) | (int(datas[ii][1]) << 8)
        if ln <= B - 2:
            pid = new_rows[ii] if new_rows[ii] < k else missing[ii - n_orig]
            out.append((pid, datas[ii][2:2 + ln].tobytes()))
    return out


@pytest.mark.parametrize("shape", COMPOSE, ids=lambda s: "k%d_m%d_B%d_%s" % s)
def test_rx_rule_restatement_matches_oracle_packets(shape):
    """rx_list_rule lists exactly the blocks from which the CPU oracle recovers rx_group's deliveries, and
    its statuses 0 and 2 are rx_group's None and k == 1 payload."""
    kmax, m, B, _ = shape
    ks, groups, recs, rx, want = compose_case(kmax, m, B)
    ora = po.oracle()
    rng = np.random.default_rng(21)
    batch, expect = [], []
    for g, (orig, got) in enumerate(rx):
        extra = [r for r in recs[g] if r not in got][:2] + [got[0]]  # trailing: unused ones, and a repeat
        batch.append(merge(rng, [orig_rec(i, p) for i, p in orig], list(got) + extra))
        expect.append(opk.rx_group(ora, orig, list(got) + extra))
        assert expect[-1] == want[g]  # the trailing packets change nothing
    # groups that are not decoded
    pk, rec = groups[0], recs[0]
    k0 = ks[0]
    single = opk.tx_group(ora, m, [b"lonely packet"])
    odd = [([(i, pk[i]) for i in range(3)], []),                       # no recovery record
           ([(i, pk[i]) for i in range(k0)], [rec[0]]),                # all originals present
           ([(i, pk[i]) for i in range(k0 - 3)], [rec[1], rec[0]]),    # too few records
           ([], [single[0], single[1]]),                               # k == 1
           ([(0, b"lonely packet")], [single[0]])]                     # k == 1, the original arrived as well
    for orig, got in odd:
        batch.append(merge(rng, [orig_rec(i, p) for i, p in orig], list(got)))
        expect.append(opk.rx_group(ora, orig, got))
    ring, pkt_first, pkt_off, pkt_len = lay_out(rng, batch)
    G, P = len(batch), len(pkt_off)
    res = rx_list_rule(2, kmax, m, B, G, P, pkt_first, pkt_off, pkt_len, ring)
    assert list(res["info"][:, 0]) == [1] * len(rx) + [0, 0, 0, 2, 0]
    assert list(res["summary"]) == [len(rx), sum(ks), 4, 1, 0, 0, 0, 0]
    assert list(res["slot_group"][:len(rx)]) == list(range(len(rx)))
    for slot in range(len(rx)):
        assert deliveries(ora, B, ring, res, slot) == expect[slot], slot
    for g in range(len(rx), G):
        status, first_rec = int(res["info"][g, 0]), int(res["info"][g, 7])
        if status == 2:
            o, ln = int(pkt_off[first_rec]), int(pkt_len[first_rec])
            assert expect[g] == [(0, ring[o + 2:o + ln].tobytes())]
        else:
            assert status == 0 and expect[g] is None
    # the same groups in a bucket that does not hold them
    res = rx_list_rule(2, kmax, m + 1, B, G, P, pkt_first, pkt_off, pkt_len, ring)
    assert list(res["info"][:, 0]) == [3] * len(rx) + [0, 0, 0, 2, 0] and res["summary"][0] == 0
    assert not res["off"].any() and (res["slot_group"] == -1).all() and not res["first"].any()


# ---------------------------------------------------------------- GPU: kernel against the rule

SIZES = [0, 1, 2, 63, 64, 65, 128, 300, MAXP, MAXP + 1]
CONFIGS = [(2, 3, 4, 16), (64, 64, 32, 24), (255, 255, 1, 8)]  # kmin, kmax, m, B


def sized_batch(rng, cfg, G, start, small=False):
    """G groups of the configuration; group i has SIZES[(start + i) % len(SIZES)] records -- with `small`,
    only the groups around the scan's tile and pass boundaries do, the others 0..4."""
    kmin, kmax, m, B = cfg
    edge = {0, SCAN_TILE - 1, SCAN_TILE, SCAN_PASS - 1, SCAN_PASS, G - 1}
    batch = []
    for i in range(G):
        k = kmin + (start + i) % (kmax - kmin + 1)
        n = SIZES[(start + i) % len(SIZES)] if not small or i in edge else int(rng.integers(0, 5))
        batch.append(sized_group(rng, k, m, B, n))
    return batch


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "k%d_%d_m%d_B%d" % c)
def test_rx_list_matches_rule(sh, cfg):
    kmin, kmax, m, B = cfg
    rng = np.random.default_rng(kmax * 7 + m)
    sh.batch_errors()
    listed_sizes = set()
    for G, start, small in [(1, 7, False), (1, 9, False), (4, 6, False), (5, 3, False), (len(SIZES), 0, False),
                            (SCAN_TILE + 1, 0, False), (SCAN_PASS + 1, 4, True)]:
        batch = sized_batch(rng, cfg, G, start, small)
        ring, pkt_first, pkt_off, pkt_len = lay_out(rng, batch)
        P = len(pkt_off)
        assert P == 0 or int((pkt_off + pkt_len).max()) == len(ring)  # a record ends exactly at ring_bytes
        assert P < 16 or set(int(v) % 8 for v in pkt_off[:P]) == set(range(8))
        want = rx_list_rule(kmin, kmax, m, B, G, P, pkt_first, pkt_off, pkt_len, ring)
        for g in range(G):
            if want["info"][g, 0] == 1:
                listed_sizes.add(len(batch[g]))
            if len(batch[g]) > MAXP:
                assert want["info"][g, 0] == -1
        for variant in (0, 1):
            rc, got = run_rx(sh, kmin, kmax, m, B, G, P, pkt_first, pkt_off, pkt_len, ring, variant)
            assert rc == 0
            assert_same(got, want, (G, start, variant))
            assert sh.batch_errors() == want["summary"][5]
    # every size from k records up was listed at least once
    assert listed_sizes >= {n for n in SIZES if kmax <= n <= MAXP}, listed_sizes
    assert sh.batch_errors() == 0


# ---------------------------------------------------------------- GPU: every status, every malformed kind

def status_batch():
    """(names, groups of records, edits of the CSR and length arrays) for kmin..kmax = 4..8, m = 4, B = 16."""
    rng = np.random.default_rng(40)
    m, B = 4, 16

    def body(ln):
        return rng.integers(0, 256, size=ln, dtype=np.uint8).tobytes()

    def group(k, orig_ids, rec_ids, gm=m, gB=B):
        return [orig_rec(i, body(int(rng.integers(0, gB - 1)))) for i in orig_ids] + \
               [recov_rec(r, k, gm, body(gB)) for r in rec_ids]

    good = lambda: group(6, [4, 0, 2, 5], [7, 9])  # noqa: E731
    cases = [
        ("good", good(), 1),
        ("no recovery record", group(6, [0, 1, 2], []), 0),
        ("all originals present", group(5, [0, 1, 2, 3, 4], [5]), 0),
        ("too few records", group(6, [0, 1, 2], [6, 7]), 0),
        ("good", good(), 1),
        ("k == 1", [bytes([1, 0]) + body(9), bytes([1, 0]) + body(9)], 2),
        ("k == 1 with an original", [orig_rec(0, body(9)), bytes([1, 0]) + body(9)], 0),
        ("k < kmin", group(3, [1], [3, 4]), 3),
        ("k > kmax", group(9, list(range(7)), [9, 10]), 3),
        ("another m", group(6, [0, 1, 2, 3], [6, 7], gm=5), 3),
        ("another B", group(6, [0, 1, 2, 3], [6, 7], gB=24), 3),
        ("good", good(), 1),
        ("mismatched c", group(6, [0, 1, 2, 3], [6]) + [recov_rec(8, 7, m, body(B))], -1),
        ("duplicate original id", group(6, [0, 1, 1, 3], [6, 7]), -1),
        ("duplicate recovery id inside use", group(6, [0, 1, 2, 3], [6, 6, 7]), -1),
        ("duplicate recovery id after use", group(6, [0, 1, 2, 3], [6, 7, 6]), 1),
        ("bad len inside use", group(6, [0, 1, 2, 3], [6]) + [recov_rec(7, 6, m, body(8))] + group(6, [], [8]), -1),
        ("original longer than the block", [orig_rec(0, body(B - 1))] + group(6, [1, 2, 3], [6, 7]), -1),
        ("original with c >= k", [orig_rec(0, body(3), c=6)] + group(6, [1, 2, 3], [6, 7]), -1),
        ("recovery id past k + m", group(6, [0, 1, 2, 3], [6, 10]), -1),
        ("B not a multiple of 8", group(6, [0, 1, 2, 3], [6, 7], gB=12), -1),
        ("B < 8", group(6, [0, 1, 2, 3], [6, 7], gB=4), -1),
        ("last recovery record of 2 bytes", group(6, [0, 1, 2, 3], [6, 7]) + [bytes([8, 5])], -1),
        ("k + m > 256", group(250, list(range(248)), [250, 251], gm=7), -1),
        ("good", good(), 1),
        ("a record of 1 byte", good(), -1),
        ("a span past the ring", good(), -1),
        ("a span before the ring", good(), -1),
        ("good", good(), 1),
        ("a CSR span that runs backwards", good(), -1),
        ("good", good(), 1),
        ("a CSR span past packets", good(), -1),
    ]
    return m, B, cases


@pytest.mark.gpu
def test_rx_every_status_and_malformed_kind(sh):
    m, B, cases = status_batch()
    kmin, kmax = 4, 8
    names = [c[0] for c in cases]
    rng = np.random.default_rng(41)
    ring, pkt_first, pkt_off, pkt_len = lay_out(rng, [c[1] for c in cases])
    G, P = len(cases), len(pkt_off)
    g = names.index("a record of 1 byte")
    pkt_len[pkt_first[g] + 2] = 1
    p = int(pkt_first[names.index("a span past the ring")]) + 4  # a recovery record: one byte too long
    pkt_len[p] = len(ring) - pkt_off[p] + 1
    pkt_off[int(pkt_first[names.index("a span before the ring")]) + 1] = -1
    g = names.index("a CSR span that runs backwards")
    pkt_first[g] = pkt_first[g + 1] + 2  # (the group in front of it now takes two records of the one behind it)
    assert names[g - 1] == names[g + 1] == "good"
    pkt_first[G] = P + 1
    want = rx_list_rule(kmin, kmax, m, B, G, P, pkt_first, pkt_off, pkt_len, ring)
    status = [int(v) for v in want["info"][:, 0]]
    back = names.index("a CSR span that runs backwards")
    for i, (name, _, expected) in enumerate(cases):
        if i != back - 1:  # (that one now holds 14 records: whatever the rule makes of them)
            assert status[i] == expected, (i, name, status[i])
    n_bad = sum(1 for s in status if s == -1)
    assert n_bad == sum(1 for c in cases if c[2] == -1) + (status[back - 1] == -1) and n_bad >= 16
    assert want["summary"][0] >= 6
    sh.batch_errors()
    for variant in (0, 1):
        rc, got = run_rx(sh, kmin, kmax, m, B, G, P, pkt_first, pkt_off, pkt_len, ring, variant, ring_bytes=len(ring))
        assert rc == 0
        assert_same(got, want, variant)
        assert sh.batch_errors() == n_bad
        assert sh.batch_errors() == 0


@pytest.mark.gpu
def test_rx_overlapping_spans_stop_at_the_capacity(sh):
    """Step 9: spans that overlap list the same records more than once; the groups whose blocks would end
    past the capacity are malformed and nothing is written past it."""
    rng = np.random.default_rng(50)
    k, m, B = 6, 4, 16
    batch = [sized_group(rng, k, m, B, 8) for _ in range(3)]
    ring, _, pkt_off, pkt_len = lay_out(rng, batch)
    P = len(pkt_off)
    # groups 0..2, then group 3 runs backwards (24 -> 0) and groups 4..6 repeat the spans, and so on
    pkt_first = np.array([0, 8, 16, 24, 0, 8, 16, 24, 0, 8, 16, 24], np.int32)
    G = len(pkt_first) - 1
    want = rx_list_rule(2, k, m, B, G, P, pkt_first, pkt_off, pkt_len, ring)
    assert want["summary"][0] == 4 and want["summary"][1] == 24 == min(P, G * k)  # capacity: 24 blocks
    assert list(want["info"][:, 0]) == [1, 1, 1, -1, 1, -1, -1, -1, -1, -1, -1]
    sh.batch_errors()
    rc, got = run_rx(sh, 2, k, m, B, G, P, pkt_first, pkt_off, pkt_len, ring, 0)
    assert rc == 0
    assert_same(got, want, "overlap")
    assert sh.batch_errors() == 7


# ---------------------------------------------------------------- GPU: round trip on the device

def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", COMPOSE, ids=lambda s: "k%d_m%d_B%d_%s" % s)
def test_rx_round_trip_on_the_device(sh, shape):
    """The sender chain of test_wire's round trip writes the recovery records into the ring, the surviving
    originals' records are uploaded beside them, and the receiver's host supplies only the CSR, pkt_off and
    pkt_len: rx_list_batch -> frame_batch -> decode_batch_out_var -> unframe_batch delivers rx_group's lists,
    with d_summary read back (a) and with upper bounds and no readback (b)."""
    import torch
    kmax, m, B, family = shape
    assert sh.path(kmax, m, B) == family
    ks, groups, recs, rx, want = compose_case(kmax, m, B)
    G, S = len(ks), 3 + B
    rng = np.random.default_rng(15)
    sh.batch_errors()
    first = np.concatenate([[0], np.cumsum(ks)]).astype(np.int32)
    total = int(first[-1])
    dfirst = _dev(first)
    # the ring: the surviving originals' records and two groups that are not decoded, then the wire region
    idle = [[orig_rec(i, b"idle %d" % i) for i in range(3)],      # no recovery record: skipped
            [bytes([1, 0]) + b"single packet group"]]             # the k == 1 form
    items = [(orig_rec(i, p), 0) for orig, _ in rx for i, p in orig] + [(r, 0) for grp in idle for r in grp]
    front, front_off = _pack(items, rng)
    wire_off = len(front) + 5
    ring = torch.from_numpy(np.concatenate([front, np.full(5 + G * m * S, GAP, np.uint8)])).cuda()
    # sender
    payload, off = _pack([(p, 0) for pk in groups for p in pk], rng)
    length = np.array([len(p) for pk in groups for p in pk], np.int32)
    blocks = torch.zeros((total, B), dtype=torch.uint8, device="cuda")
    rec = torch.zeros((G, m, B), dtype=torch.uint8, device="cuda")
    assert sh.frame_batch(B, total, _dev(payload), len(payload), _dev(off), _dev(length), None, blocks) == 0
    assert sh.encode_batch_var(kmax, m, B, G, dfirst, total, blocks, rec) == 0
    assert sh.wire_emit_batch(kmax, m, B, G, dfirst, total, rec, ring[wire_off:]) == 0
    # receiver: where each record lies and which group it belongs to. Batch order: g0, idle0, g1, idle1, g2, ...
    order, o = [], 0
    per_group = []
    for g, (orig, pkts) in enumerate(rx):
        a = []
        for _ in orig:
            a.append((int(front_off[o]), len(items[o][0])))
            o += 1
        b = [(wire_off + (g * m + (pkt[0] - ks[g])) * S, S) for pkt in pkts]
        per_group.append(merge(rng, a, b))
    idle_spans = []
    for grp in idle:
        idle_spans.append([(int(front_off[o + j]), len(r)) for j, r in enumerate(grp)])
        o += len(grp)
    for g in range(G):
        order.append((g, per_group[g]))
        if g < len(idle_spans):
            order.append((None, idle_spans[g]))
    GA = len(order)
    pkt_first = np.concatenate([[0], np.cumsum([len(s) for _, s in order])]).astype(np.int32)
    pkt_off = np.array([s[0] for _, sp in order for s in sp], np.int64)
    pkt_len = np.array([s[1] for _, sp in order for s in sp], np.int32)
    P = len(pkt_off)
    listed = [g for g, _ in order if g is not None]
    cap = sh.rx_list_capacity(GA, P, kmax)
    guards = guarded_outputs(GA, cap, variant=0)
    tt = {name: gd.tensor({np.int32: torch.int32, np.int64: torch.int64, np.uint8: torch.uint8}[dt])
          for name, (gd, dt) in guards.items()}
    info, lfirst, slot_group, summary = tt["info"].view(GA, INFO), tt["first"], tt["slot_group"], tt["summary"]
    loff, llen, lraw, lrows = tt["off"], tt["len"], tt["raw"], tt["rows"]
    scratch = Guarded(sh.rx_list_scratch_bytes(GA, P), 8)
    d_in = [Guarded(4 * (GA + 1), 4, pkt_first), Guarded(8 * P, 8, pkt_off), Guarded(4 * P, 12, pkt_len)]
    sent = ring.cpu().numpy()
    assert sh.rx_list_batch(2, kmax, m, B, GA, P, d_in[0].ptr, d_in[1].ptr, d_in[2].ptr, ring, ring.numel(),
                            info, lfirst, slot_group, loff, llen, lraw, lrows, summary, scratch.ptr) == 0
    emax = min(kmax, m)

    def receive(n_groups, n_blocks):
        """frame -> decode -> unframe over the lists, with these bounds; the deliveries per slot."""
        blocks = torch.zeros((n_blocks, B), dtype=torch.uint8, device="cuda")
        assert sh.frame_batch(B, n_blocks, ring, ring.numel(), loff, llen, lraw, blocks) == 0
        slots = n_groups * emax
        out = torch.full((n_groups, emax, B), 0x77, dtype=torch.uint8, device="cuda")
        out_rows = torch.zeros((n_groups, emax), dtype=torch.uint8, device="cuda")
        count = torch.full((n_groups,), -7, dtype=torch.int32, device="cuda")
        assert sh.decode_batch_out_var(kmax, m, B, n_groups, lfirst, n_blocks, blocks, lrows, out, out_rows,
                                       count) == 0
        pcap = slots * (B - 2)
        pay = torch.full((pcap,), CANARY, dtype=torch.uint8, device="cuda")
        doff = torch.zeros(slots + 1, dtype=torch.int64, device="cuda")
        dlen = torch.zeros(slots, dtype=torch.int32, device="cuda")
        scr = torch.zeros(sh.unframe_scratch_bytes(n_groups, emax), dtype=torch.uint8, device="cuda")
        assert sh.unframe_batch(B, n_groups, emax, emax, out, count, pay, pcap, doff, dlen, scr) == 0
        errors = sh.batch_errors()
        pay, doff, dlen, out_rows = pay.cpu().numpy(), doff.cpu().numpy(), dlen.cpu().numpy(), out_rows.cpu().numpy()
        got = [[(int(out_rows[s, i]), pay[doff[t]:doff[t] + dlen[t]].tobytes())
                for i in range(emax) for t in [s * emax + i] if dlen[t] >= 0] for s in range(n_groups)]
        return got, count.cpu().numpy(), errors

    # (a) the one readback: d_summary
    n_listed, n_blocks = (int(v) for v in summary.cpu().numpy()[:2])
    assert (n_listed, n_blocks) == (G, total)
    got, count, errors = receive(n_listed, n_blocks)
    assert errors == 0
    sg = slot_group.cpu().numpy()
    assert [order[int(sg[s])][0] for s in range(n_listed)] == listed and (sg[n_listed:] == -1).all()
    for s in range(n_listed):
        assert got[s] == want[listed[s]], s
    st = info.cpu().numpy()[:, 0]
    assert [int(st[i]) for i, (g, _) in enumerate(order) if g is None] == [0, 2]
    # (b) no readback: upper bounds
    got, count, errors = receive(GA, cap)
    assert errors == GA - n_listed
    for s in range(n_listed):
        assert got[s] == want[listed[s]], s
    assert (count[n_listed:] == -1).all() and all(not got[s] for s in range(n_listed, GA))
    # nothing outside the outputs was written, and the inputs are as they were
    for gd, dt in guards.values():
        gd.read(dt)
    scratch.read(np.uint8)
    assert all(d.unchanged() for d in d_in)
    assert np.array_equal(ring.cpu().numpy(), sent) and np.array_equal(sent[:len(front)], front)


# ---------------------------------------------------------------- GPU: the binding on tensors, in a graph

@pytest.mark.gpu
def test_rx_python_binding_on_tensors_and_graph_replay(sh):
    """Two replays of a captured listing call, each on a changed ring, give the rule's outputs."""
    import torch
    kmin, kmax, m, B = 4, 8, 4, 16
    rng = np.random.default_rng(60)
    ks = [int(v) for v in rng.integers(kmin, kmax + 1, size=37)]
    batch = [sized_group(rng, k, m, B, k + 2) for k in ks]
    ring, pkt_first, pkt_off, pkt_len = lay_out(rng, batch)
    G, P = len(batch), len(pkt_off)
    cap = sh.rx_list_capacity(G, P, kmax)
    s = torch.cuda.Stream()
    d_ring = _dev(ring)
    d_in = [_dev(pkt_first), _dev(pkt_off), _dev(pkt_len)]
    guards = guarded_outputs(G, cap, variant=0)
    t = {name: gd.tensor({np.int32: torch.int32, np.int64: torch.int64, np.uint8: torch.uint8}[dt])
         for name, (gd, dt) in guards.items()}
    t["info"] = t["info"].view(G, INFO)
    scratch = Guarded(sh.rx_list_scratch_bytes(G, P), 8).tensor(torch.uint8)
    torch.cuda.synchronize()

    def run():
        assert sh.rx_list_batch(kmin, kmax, m, B, G, P, d_in[0], d_in[1], d_in[2], d_ring, d_ring.numel(), t["info"],
                                t["first"], t["slot_group"], t["off"], t["len"], t["raw"], t["rows"], t["summary"],
                                scratch) == 0

    def check(ring_now, tag):
        want = rx_list_rule(kmin, kmax, m, B, G, P, pkt_first, pkt_off, pkt_len, ring_now)
        got = {name: gd.read(dt) for name, (gd, dt) in guards.items()}  # (checks the canaries)
        got["info"] = got["info"].reshape(G, INFO)
        assert_same(got, want, tag)
        assert np.array_equal(d_ring.cpu().numpy(), ring_now)
        assert all(np.array_equal(d.cpu().numpy(), a) for d, a in zip(d_in, (pkt_first, pkt_off, pkt_len)))
        return want

    sh.batch_errors()
    with torch.cuda.stream(s):
        run()  # loads the kernels' code and creates the stream's error counter before the capture
    s.synchronize()
    want = check(ring, "eager")
    assert want["summary"][0] == G
    # a captured graph replays on hardware queues of its own: the runtime needs its default of four
    queues = os.environ.get("GPU_MAX_HW_QUEUES")
    assert queues is None or int(queues) >= 4, queues
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        run()
    malformed = 0
    for rep in range(2):
        # another ring under the same offsets: every body changes, and the first recovery record of group
        # `rep` gets another c
        ring2 = ring.copy()
        ring2[:] = rng.integers(0, 256, size=len(ring), dtype=np.uint8)
        for p in range(P):
            ring2[pkt_off[p]:pkt_off[p] + min(3, pkt_len[p])] = ring[pkt_off[p]:pkt_off[p] + min(3, pkt_len[p])]
        g = rep
        for p in range(pkt_first[g], pkt_first[g + 1]):
            if ring2[pkt_off[p]] > ring2[pkt_off[p] + 1]:
                ring2[pkt_off[p] + 1] ^= 1 + rep
                break
        d_ring.copy_(torch.from_numpy(ring2))
        for v in t.values():
            v.fill_(5)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        want = check(ring2, rep)
        assert want["summary"][0] < G
        malformed += int(want["summary"][5])
    assert sh.batch_errors(s.cuda_stream) == malformed
