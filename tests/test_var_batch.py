"""Var-k batches (include/cauchy_256_batch.h: cauchy_256_encode_batch_var /
cauchy_256_decode_batch_out_var): groups with per-group k, packed CSR-style by first[], in one launch.

Expected bytes come from the CPU oracle run per group at that group's own k_g, never from the
library's uniform calls. The premise -- the generator's column x is the same for every k, so coding
k blocks equals coding them padded with zero blocks to any larger k -- is checked on the CPU.
"""
import functools

import numpy as np
import pytest

from oracle import pyoracle as po

CFG = 0x5EED
PAD_MS = [1, 2, 3, 4, 5, 6, 7, 8, 10, 16, 32, 40, 66, 76, 136, 200, 254]


def _pad_ks(m):
    kfull = 256 - m
    return sorted({k for k in (2, 3, 7, kfull // 2, (6 * kfull) // 10, kfull - 1, kfull) if 2 <= k <= kfull})


@pytest.mark.parametrize("m", PAD_MS)
def test_zero_padding_identity(m):
    """encode(k, m, data) == encode(256 - m, m, data || zero blocks), byte for byte (k >= 2)."""
    codec = po.reference() or po.oracle()
    B, kfull = 64, 256 - m
    for k in _pad_ks(m):
        data = po.fill_group(k + 1000 * m, k, B, CFG)
        padded = np.zeros((kfull, B), np.uint8)
        padded[:k] = data
        rc0, a = codec.encode(k, m, data, B)
        rc1, b = codec.encode(kfull, m, padded, B)
        assert rc0 == 0 and rc1 == 0
        assert np.array_equal(a, b), (k, m)


def test_var_calls_reject_bad_parameters_without_gpu():
    """Host-checked parameters return -1 before anything touches the GPU."""
    import shorthair_amd as sh
    enc, dec = sh.lib.cauchy_256_encode_batch_var, sh.lib.cauchy_256_decode_batch_out_var
    bad = [(1, 4, 256, 4, 4), (256, 1, 256, 4, 4), (200, 57, 256, 4, 4), (28, 4, 252, 4, 4),
           (28, 4, 256, -1, 0), (28, 4, 256, 4, -1), (28, 4, 256, 4, 4 * 28 + 1), (28, 0, 256, 4, 4)]
    for kmax, m, B, G, total in bad:
        assert enc(kmax, m, B, G, None, total, None, None, None) == -1, (kmax, m, B, G, total)
        assert dec(kmax, m, B, G, None, total, None, None, None, None, None, None) == -1
    assert dec(28, 1, 256, 4, None, 8, None, None, None, None, None, None) == -1  # decode: m >= 2


# ---------------------------------------------------------------- cases, built once per shape

SHAPES = [
    (28, 4, 256, 37),     # compile-time: 16 groups per 128-column tile, partial last tile
    (64, 16, 1400, 7),    # compile-time: groups split across tiles
    (60, 16, 136, 19),    # compile-time: kmax below the compiled K; shifted tail chunk
    (200, 32, 1400, 5),   # compile-time: headline shape
    (190, 66, 1336, 4),   # compile-time: nine-row parts
    (50, 10, 1000, 7),    # tile
    (17, 5, 520, 9),      # tile: searched m <= 6 tables
    (100, 140, 128, 5),   # tile: row launches for m > 128
    (20, 5, 64, 11),      # generic
    (12, 7, 8, 33),       # generic: smallest block
    (20, 2, 1400, 5),     # m = 2
]
PATHS = {(28, 4, 256): "fixed", (64, 16, 1400): "fixed", (60, 16, 136): "fixed", (200, 32, 1400): "fixed",
         (190, 66, 1336): "fixed", (50, 10, 1000): "tile", (17, 5, 520): "tile", (100, 140, 128): "tile",
         (20, 5, 64): "generic", (12, 7, 8): "generic"}


def _ks(kmax, groups, seed, uniform=False):
    if uniform:
        return [kmax] * groups
    rng = np.random.default_rng(seed)
    ks = [int(v) for v in rng.integers(2, kmax + 1, size=groups)]
    ks[0], ks[1] = 2, kmax                    # both ends, and two adjacent groups that differ
    ks[2] = max(2, (6 * kmax) // 10 - 1)      # below 0.6 kmax
    return ks


class Case:
    """One batch: per-group inputs, the oracle's recovery blocks and one decode pattern per group.
    es: the erasure count of every group instead of the drawn ones. force_rows: {group: recovery
    rows that group's pattern must use}; its e is drawn from their number up. Without the two, a
    case holds the bytes it always held."""

    def __init__(self, kmax, m, B, groups, seed, uniform=False, ks=None, es=None, force_rows=None):
        ora = po.oracle()
        self.kmax, self.m, self.B, self.G = kmax, m, B, groups
        self.ks = ks if ks is not None else _ks(kmax, groups, seed, uniform)
        self.first = np.concatenate([[0], np.cumsum(self.ks)]).astype(np.int32)
        self.total = int(self.first[-1])
        self.data = [po.fill_group(seed * 1000 + g, k, B, CFG) for g, k in enumerate(self.ks)]
        self.rec = []
        for k, d in zip(self.ks, self.data):
            if not 2 <= k <= kmax:  # a malformed group (test_var_malformed_groups): nothing to expect
                self.rec.append(None)
                continue
            rc, out = ora.encode(k, m, d, B)
            assert rc == 0
            self.rec.append(out)
        self.packed = np.concatenate(self.data) if self.total else np.zeros((0, B), np.uint8)
        if m < 2:
            return
        # decode: e_g random in 0..min(k_g, m) with both ends forced, blocks in shuffled array order
        rng = np.random.default_rng(seed + 77)
        emax = min(kmax, m)
        self.blocks = np.zeros((self.total, B), np.uint8)
        self.rows = np.zeros(self.total, np.uint8)
        self.out = np.zeros((groups, emax, B), np.uint8)
        self.out_rows = np.zeros((groups, emax), np.uint8)
        self.count = np.zeros(groups, np.int32)
        for g, k in enumerate(self.ks):
            f = int(self.first[g])
            if self.rec[g] is None:
                self.blocks[f:f + k] = self.data[g]
                self.rows[f:f + k] = np.arange(k) % 256
                self.count[g] = -1
                continue
            top = min(k, m)
            forced = sorted((force_rows or {}).get(g, ()))
            if es is not None:
                e = int(es[g])
                assert len(forced) <= e <= top
            elif forced:
                e = int(rng.integers(len(forced), top + 1))
            else:
                e = 0 if g == 3 else (top if g in (0, 1) else int(rng.integers(0, top + 1)))
            lost = set(int(x) for x in rng.choice(k, size=e, replace=False))
            if forced:
                free = [y for y in range(m) if y not in forced]
                ys = sorted(forced + [int(y) for y in rng.choice(free, size=e - len(forced), replace=False)])
            else:
                ys = sorted(int(y) for y in rng.choice(m, size=e, replace=False))
            items = [(x, self.data[g][x]) for x in range(k) if x not in lost] + [(k + y, self.rec[g][y]) for y in ys]
            order = rng.permutation(k)
            items = [items[i] for i in order]
            for i, (row, blk) in enumerate(items):
                self.blocks[f + i] = blk
                self.rows[f + i] = row
            datas = [blk.copy() for _, blk in items]
            rc, new_rows = ora.decode(k, m, datas, [r for r, _ in items], B)
            assert rc == 0
            slots = [i for i, (row, _) in enumerate(items) if row >= k]  # recovery blocks in array order
            self.count[g] = e
            for i, s in enumerate(slots):
                self.out[g, i] = datas[s]
                self.out_rows[g, i] = new_rows[s]
            assert [int(r) for r in self.out_rows[g, :e]] == sorted(lost)


@functools.lru_cache(maxsize=None)
def case(kmax, m, B, groups, uniform=False):
    return Case(kmax, m, B, groups, seed=kmax * 7 + m, uniform=uniform)


@pytest.fixture(scope="module")
def sh():
    import torch
    import shorthair_amd
    assert shorthair_amd.cauchy_256_init() == 0
    torch.cuda.init()
    return shorthair_amd


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _encode(sh, c, first=None, total=None):
    import torch
    rec = torch.full((c.G, c.m, c.B), 0x5A, dtype=torch.uint8, device="cuda")
    first = c.first if first is None else first
    rc = sh.encode_batch_var(c.kmax, c.m, c.B, c.G, _dev(first), c.total if total is None else total,
                             _dev(c.packed), rec)
    assert rc == 0
    torch.cuda.synchronize()
    return rec.cpu().numpy()


def _decode(sh, c):
    import torch
    emax = min(c.kmax, c.m)
    out = torch.zeros((c.G, emax, c.B), dtype=torch.uint8, device="cuda")
    out_rows = torch.zeros((c.G, emax), dtype=torch.uint8, device="cuda")
    count = torch.full((c.G,), -7, dtype=torch.int32, device="cuda")
    rc = sh.decode_batch_out_var(c.kmax, c.m, c.B, c.G, _dev(c.first), c.total, _dev(c.blocks), _dev(c.rows),
                                 out, out_rows, count)
    assert rc == 0
    torch.cuda.synchronize()
    return out.cpu().numpy(), out_rows.cpu().numpy(), count.cpu().numpy()


def _check_decode(c, out, out_rows, count, skip=()):
    for g in range(c.G):
        if g in skip:
            continue
        e = int(c.count[g])
        assert count[g] == e, g
        assert np.array_equal(out_rows[g, :e], c.out_rows[g, :e]), g
        assert np.array_equal(out[g, :e], c.out[g, :e]), g


# ---------------------------------------------------------------- GPU

@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES + [(30, 1, 256, 9)], ids=lambda s: "k%d_m%d_B%d_G%d" % s)
def test_var_encode_matches_oracle_per_group(sh, shape):
    kmax, m, B, groups = shape
    if (kmax, m, B) in PATHS:
        assert sh.path(kmax, m, B) == PATHS[(kmax, m, B)]
    c = case(*shape)
    assert set(c.ks) >= {2, kmax} and min(c.ks[2:3]) < 0.6 * kmax and c.ks[0] != c.ks[1]
    sh.batch_errors()
    got = _encode(sh, c)
    for g in range(groups):
        assert np.array_equal(got[g], c.rec[g]), (g, c.ks[g])
    assert sh.batch_errors() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "k%d_m%d_B%d_G%d" % s)
def test_var_decode_matches_oracle_per_group(sh, shape):
    c = case(*shape)
    assert 0 in c.count and any(c.count[g] == min(c.ks[g], c.m) for g in range(c.G))
    sh.batch_errors()
    out, out_rows, count = _decode(sh, c)
    _check_decode(c, out, out_rows, count)
    assert sh.batch_errors() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(28, 4, 256, 6), (200, 32, 1400, 3)], ids=lambda s: "k%d_m%d_B%d_G%d" % s)
def test_var_uniform_k_matches_oracle(sh, shape):
    """Every k_g = kmax: the var calls give the oracle's bytes too."""
    c = case(*shape, uniform=True)
    got = _encode(sh, c)
    for g in range(c.G):
        assert np.array_equal(got[g], c.rec[g]), g
    _check_decode(c, *_decode(sh, c))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(28, 4, 256, 8192), (60, 16, 136, 8192)], ids=lambda s: "k%d_m%d_B%d_G%d" % s)
def test_var_decode_many_groups(sh, shape):
    """From 8,192 groups on, the decode setup runs its multi-group kernels (m <= 6: eight lanes per
    group; m >= 7 with at most 16 erasures: sixteen). Every group's recovered blocks must be the
    erased originals in ascending order -- what the oracle's decode returns, checked on a sample of
    groups together with their recovery blocks."""
    import torch
    kmax, m, B, G = shape
    ora = po.oracle()
    rng = np.random.default_rng(kmax + m)
    ks = rng.integers(2, kmax + 1, size=G)
    ks[0], ks[1] = 2, kmax
    first = np.concatenate([[0], np.cumsum(ks)]).astype(np.int32)
    total = int(first[-1])
    data = rng.integers(0, 256, size=(total, B), dtype=np.uint8)
    dfirst, ddata = _dev(first), _dev(data)
    rec = torch.zeros((G, m, B), dtype=torch.uint8, device="cuda")
    sh.batch_errors()
    assert sh.encode_batch_var(kmax, m, B, G, dfirst, total, ddata, rec) == 0
    rec_np = rec.cpu().numpy()
    sample = [0, 1] + [int(g) for g in rng.choice(G, size=30, replace=False)]
    for g in sample:
        rc, exp = ora.encode(int(ks[g]), m, data[first[g]:first[g + 1]], B)
        assert rc == 0 and np.array_equal(rec_np[g], exp), g
    emax = min(kmax, m)
    rows = np.zeros(total, np.uint8)
    idx = np.zeros(total, np.int64)          # into [data ; rec]
    want_rows = np.zeros((G, emax), np.uint8)
    want_src = np.zeros((G, emax), np.int64)  # block of `data` each output must equal
    count = np.zeros(G, np.int32)
    for g in range(G):
        k, f = int(ks[g]), int(first[g])
        e = int(rng.integers(0, min(k, m) + 1))
        lost = np.sort(rng.choice(k, size=e, replace=False))
        ys = np.sort(rng.choice(m, size=e, replace=False))
        r = np.concatenate([np.setdiff1d(np.arange(k), lost), k + ys])[rng.permutation(k)]
        rows[f:f + k] = r
        idx[f:f + k] = np.where(r < k, f + r, total + g * m + (r - k))
        count[g] = e
        want_rows[g, :e] = lost
        want_src[g, :e] = f + lost
    blocks = np.concatenate([data, rec_np.reshape(G * m, B)])[idx]
    for g in sample:  # the oracle's decode agrees with the expectation used for every group
        k, f, e = int(ks[g]), int(first[g]), int(count[g])
        datas = [blocks[f + i].copy() for i in range(k)]
        rc, new_rows = ora.decode(k, m, datas, [int(x) for x in rows[f:f + k]], B)
        slots = [i for i in range(k) if rows[f + i] >= k]
        assert rc == 0 and [new_rows[i] for i in slots] == want_rows[g, :e].tolist()
        assert all(np.array_equal(datas[s], data[want_src[g, i]]) for i, s in enumerate(slots))
    out = torch.zeros((G, emax, B), dtype=torch.uint8, device="cuda")
    out_rows = torch.zeros((G, emax), dtype=torch.uint8, device="cuda")
    cnt = torch.full((G,), -7, dtype=torch.int32, device="cuda")
    assert sh.decode_batch_out_var(kmax, m, B, G, dfirst, total, _dev(blocks), _dev(rows), out, out_rows, cnt) == 0
    assert sh.batch_errors() == 0
    assert np.array_equal(cnt.cpu().numpy(), count)
    used = np.arange(emax)[None, :] < count[:, None]
    assert np.array_equal(out_rows.cpu().numpy()[used], want_rows[used])
    assert np.array_equal(out.cpu().numpy()[used], data[want_src[used]])


def _malformed(first, kmax, total):
    return [g for g in range(len(first) - 1)
            if not (first[g] >= 0 and first[g + 1] <= total and 2 <= first[g + 1] - first[g] <= kmax)]


def _bad_case(name):
    """(Case, first[] handed to the library, malformed groups) at (28, 4, 256, 12)."""
    kmax, m, B, groups = 28, 4, 256, 12
    ks = _ks(kmax, groups, {"k1": 5, "kmax_plus_1": 6, "first_past_total": 8}[name])
    if name == "k1":
        ks[4] = 1
    if name == "kmax_plus_1":
        ks[7] = kmax + 1
    c = Case(kmax, m, B, groups, seed=900 + len(name), ks=ks)
    assert c.total <= groups * kmax
    first = c.first.copy()
    if name == "first_past_total":
        first[5] = c.total + 9
    bad = _malformed(first, kmax, c.total)
    assert bad == {"k1": [4], "kmax_plus_1": [7], "first_past_total": [4, 5]}[name]
    return c, first, bad


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["k1", "kmax_plus_1", "first_past_total"])
def test_var_malformed_groups(sh, name):
    """Malformed groups read nothing and write nothing outside the outputs (canaries on both sides),
    get zeros (encode) or count -1 (decode) and are counted; their neighbours code correctly."""
    import torch
    c, first, bad = _bad_case(name)
    kmax, m, B, groups = c.kmax, c.m, c.B, c.G
    emax = min(kmax, m)
    PADB = 4096

    def guarded(n):
        buf = torch.full((PADB + n + PADB,), 0xA5, dtype=torch.uint8, device="cuda")
        return buf, buf[PADB:PADB + n]

    def inner(buf):
        b = buf.cpu().numpy()
        assert (b[:PADB] == 0xA5).all() and (b[-PADB:] == 0xA5).all()
        return b[PADB:-PADB]

    dfirst, dpacked, dblocks, drows = _dev(first), _dev(c.packed), _dev(c.blocks), _dev(c.rows)
    stream = torch.cuda.current_stream().cuda_stream
    sh.batch_errors()
    # encode: the bad groups' recovery blocks are written as zeros over the 0x5A fill
    rbuf, rec = guarded(groups * m * B)
    rec.fill_(0x5A)
    assert sh.lib.cauchy_256_encode_batch_var(kmax, m, B, groups, dfirst.data_ptr(), c.total,
                                              dpacked.data_ptr(), rec.data_ptr(), stream) == 0
    assert sh.batch_errors() == len(bad)
    assert sh.batch_errors() == 0
    got = inner(rbuf).reshape(groups, m, B)
    for g in range(groups):
        if g in bad:
            assert not got[g].any(), g
        else:
            assert np.array_equal(got[g], c.rec[g]), g
    # decode
    obuf, out = guarded(groups * emax * B)
    wbuf, out_rows = guarded(groups * emax)
    cbuf, cnt = guarded(groups * 4)
    assert sh.lib.cauchy_256_decode_batch_out_var(kmax, m, B, groups, dfirst.data_ptr(), c.total,
                                                  dblocks.data_ptr(), drows.data_ptr(),
                                                  out.data_ptr(), out_rows.data_ptr(), cnt.data_ptr(), stream) == 0
    assert sh.batch_errors() == len(bad)
    assert sh.batch_errors() == 0
    count = inner(cbuf).view(np.int32)
    for g in bad:
        assert count[g] == -1, g
    _check_decode(c, inner(obuf).reshape(groups, emax, B), inner(wbuf).reshape(groups, emax), count, skip=set(bad))


@pytest.mark.gpu
def test_var_decode_replays_from_a_graph_after_reserve(sh):
    """After batch_reserve(kmax, m, B, groups) a var decode allocates nothing: it is captured into a
    graph on one stream and replays to the same bytes."""
    import torch
    c = case(28, 4, 256, 37)
    emax = min(c.kmax, c.m)
    s = torch.cuda.Stream()
    assert sh.batch_reserve(c.kmax, c.m, c.B, c.G) == 0
    assert sh.lib.cauchy_256_batch_reserve_stream(c.kmax, c.m, c.B, c.G, s.cuda_stream) == 0
    first, blocks, rows = _dev(c.first), _dev(c.blocks), _dev(c.rows)
    out = torch.zeros((c.G, emax, c.B), dtype=torch.uint8, device="cuda")
    out_rows = torch.zeros((c.G, emax), dtype=torch.uint8, device="cuda")
    count = torch.zeros((c.G,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def run():
        assert sh.decode_batch_out_var(c.kmax, c.m, c.B, c.G, first, c.total, blocks, rows, out, out_rows,
                                       count) == 0

    with torch.cuda.stream(s):
        run()  # loads the kernels' code before the capture
    s.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        run()
    for _ in range(2):
        out.zero_()
        out_rows.zero_()
        count.fill_(-7)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        _check_decode(c, out.cpu().numpy(), out_rows.cpu().numpy(), count.cpu().numpy())
