"""The batched codec calls at unaligned device pointers, with guard bytes
(include/cauchy_256_batch.h: "byte offsets inside one device allocation, no alignment required").

Every buffer of a call -- inputs and outputs alike -- sits in an allocation of its own, at a chosen
address mod 16, between two 4096-byte guards, and the whole allocation holds seeded random bytes
(equal constants would cancel under XOR). Inputs are then overwritten with the case's bytes; outputs
keep the random fill, so a stale or unwritten byte never looks right by accident. After the call one
checker compares host copies of the whole allocations with what they must be:
  1. both guards of every buffer are byte-identical to their pre-call copy,
  2. every input is byte-identical to its pre-call copy,
  3. every output byte equals the CPU oracle's (oracle/pyoracle.py, run per group), and the slots the
     header leaves untouched -- d_out[g][e_g .. emax) and d_out_rows[g][e_g .. emax) -- still hold
     their pre-call fill.
No expectation comes from the library under test.
"""
import functools

import numpy as np
import pytest

from oracle import pyoracle as po
from tests.test_var_batch import PATHS, Case, case

PAD = 4096


# ---------------------------------------------------------------- harness

def placed(nbytes, mis, rng):
    """A uint8 cuda tensor of PAD + 16 + nbytes + PAD seeded random bytes and a view of nbytes of it
    whose address is = mis (mod 16)."""
    import torch
    host = rng.integers(0, 256, size=PAD + 16 + nbytes + PAD, dtype=np.uint8)
    buf = torch.from_numpy(host).cuda()
    start = PAD + (mis - (buf.data_ptr() + PAD)) % 16
    view = buf[start:start + nbytes]
    assert view.data_ptr() % 16 == mis and PAD <= start < PAD + 16
    return buf, view


class Buf:
    """One buffer of a call: `pre` is the host copy of the whole allocation before the call, the
    buffer proper is pre[start : start + nbytes]. role "in": read-only; role "out": `want` holds the
    nbytes it must hold after the call (in-place buffers included). unit: bytes per group, for the
    failure message."""

    def __init__(self, name, role, pre, start, nbytes, dev=None, unit=1):
        self.name, self.role, self.pre, self.start, self.nbytes = name, role, pre, start, nbytes
        self.dev, self.unit, self.want = dev, unit, None

    @property
    def ptr(self):
        return self.dev.data_ptr() + self.start

    @property
    def fill(self):
        """The buffer's pre-call bytes (a copy)."""
        return self.pre[self.start:self.start + self.nbytes].copy()


def make_buf(name, role, nbytes, mis, rng, content=None, unit=1, device=True):
    """Place one buffer (device=False: a numpy stand-in whose "address" is its offset) and, for an
    input or an in-place buffer, overwrite it with `content`."""
    if content is not None:
        content = np.ascontiguousarray(content).view(np.uint8).reshape(-1)
        assert content.size == nbytes
    if device:
        import torch
        dev, view = placed(nbytes, mis, rng)
        start = view.data_ptr() - dev.data_ptr()
        if content is not None:
            view.copy_(torch.from_numpy(content))
        pre = dev.cpu().numpy()
    else:
        dev = None
        pre = rng.integers(0, 256, size=PAD + 16 + nbytes + PAD, dtype=np.uint8)
        start = PAD + mis
        if content is not None:
            pre[start:start + nbytes] = content
    if content is not None:
        assert np.array_equal(pre[start:start + nbytes], content)
    return Buf(name, role, pre, start, nbytes, dev, unit)


def _same(got, want, b, what, base=0):
    if got.shape == want.shape and np.array_equal(got, want):
        return
    assert got.shape == want.shape, "%s: %s has %s bytes, not %s" % (b.name, what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    at = int(bad[0])
    raise AssertionError("%s: %s differs in %d bytes, first at byte %d (group %d): got 0x%02x, want 0x%02x"
                         % (b.name, what, bad.size, base + at, (base + at) // b.unit, got[at], want[at]))


def check(bufs, after):
    """after: name -> host copy of the whole allocation after the call."""
    for b in bufs:  # 1. guards
        got, lo, hi = after[b.name], b.start, b.start + b.nbytes
        assert got.dtype == np.uint8 and got.shape == b.pre.shape, b.name
        _same(got[:lo], b.pre[:lo], b, "guard before", -lo)
        _same(got[hi:], b.pre[hi:], b, "guard after", b.nbytes)
    for b in bufs:  # 2. inputs stay read-only
        if b.role == "in":
            _same(after[b.name][b.start:b.start + b.nbytes], b.pre[b.start:b.start + b.nbytes], b, "read-only input")
    for b in bufs:  # 3. outputs
        if b.role == "out":
            assert b.want is not None and b.want.dtype == np.uint8 and b.want.size == b.nbytes, b.name
            _same(after[b.name][b.start:b.start + b.nbytes], b.want.reshape(-1), b, "output")


def fetch(bufs):
    import torch
    torch.cuda.synchronize()
    return {b.name: b.dev.cpu().numpy() for b in bufs}


def overlay(fill, exp, count):
    """Slots i < count[g] of every group take the oracle's bytes; the others (count 0 and -1 groups
    included) keep the pre-call fill: every stage-B family and every setup leaves them untouched."""
    want = fill.reshape(exp.shape).copy()
    used = np.arange(exp.shape[1])[None, :] < np.asarray(count)[:, None]
    want[used] = exp[used]
    return want


# ---------------------------------------------------------------- cases (oracle-built, once per shape)

class Batch:
    """A Case's arrays in batch layout, repeated `rep` times along the group axis."""

    def __init__(self, c, rep=1, with_data=True):
        self.kmax, self.m, self.B, self.G = c.kmax, c.m, c.B, c.G * rep
        self.emax = min(c.kmax, c.m)
        self.first, self.total = None, c.total * rep

        def tile(a):
            return np.tile(a, (rep,) + (1,) * (a.ndim - 1)) if rep > 1 else a

        if with_data:
            self.data = tile(c.packed)                  # [total][B]
            self.rec = tile(np.stack(c.rec))            # [G][m][B]
        if c.m >= 2:
            self.blocks, self.rows = tile(c.blocks), tile(c.rows)
            self.out, self.out_rows, self.count = tile(c.out), tile(c.out_rows), tile(c.count)
        if rep == 1:
            self.first = c.first


@functools.lru_cache(maxsize=None)
def uniform(k, m, B, G, rep=1):
    """Every k_g = k: the packed layout is the uniform [G][k][B] layout. Oracle-built per group."""
    c = case(k, m, B, G, uniform=True)
    assert c.ks == [k] * G and G >= 4 and c.count[3] == 0 and c.count[0] == min(k, m)
    return Batch(c, rep, with_data=rep == 1)


@functools.lru_cache(maxsize=None)
def nonuniform(kmax, m, B, G):
    c = case(kmax, m, B, G)
    assert len(set(c.ks)) > 1 and c.count[3] == 0
    return Batch(c)


def seed_of(*parts):
    s = 0
    for p in parts:
        for v in (p if isinstance(p, (tuple, list)) else (p,)):
            s = (s * 1000003 + int(v) + 1) % (2 ** 63)
    return s


def encode_bufs(b, mis, rng, device=True, first_mis=None):
    md, mr = mis
    bufs = []
    if first_mis is not None:
        bufs.append(make_buf("first", "in", 4 * (b.G + 1), first_mis, rng, b.first, device=device))
    bufs.append(make_buf("data", "in", b.total * b.B, md, rng, b.data, unit=b.kmax * b.B, device=device))
    rec = make_buf("recovery", "out", b.G * b.m * b.B, mr, rng, unit=b.m * b.B, device=device)
    rec.want = np.ascontiguousarray(b.rec).reshape(-1)
    bufs.append(rec)
    return bufs


def decode_out_bufs(b, mis, rng, device=True, first_mis=None):
    mb, mr, mo, mw, mc = mis
    assert mc % 4 == 0  # d_out_count is an int*
    bufs = []
    if first_mis is not None:
        bufs.append(make_buf("first", "in", 4 * (b.G + 1), first_mis, rng, b.first, device=device))
    bufs.append(make_buf("blocks", "in", b.total * b.B, mb, rng, b.blocks, unit=b.kmax * b.B, device=device))
    bufs.append(make_buf("rows", "in", b.total, mr, rng, b.rows, unit=b.kmax, device=device))
    out = make_buf("out", "out", b.G * b.emax * b.B, mo, rng, unit=b.emax * b.B, device=device)
    out.want = overlay(out.fill, b.out, b.count).reshape(-1)
    out_rows = make_buf("out_rows", "out", b.G * b.emax, mw, rng, unit=b.emax, device=device)
    out_rows.want = overlay(out_rows.fill, b.out_rows, b.count).reshape(-1)
    count = make_buf("out_count", "out", 4 * b.G, mc, rng, unit=4, device=device)
    count.want = np.ascontiguousarray(b.count.astype("<i4")).view(np.uint8)
    return bufs + [out, out_rows, count]


def inplace_bufs(b, mis, rng, device=True):
    """The j-th recovery block of a group in array order now holds out[g][j] and its row is
    out_rows[g][j]; every other block and row is byte-identical."""
    mb, mr = mis
    k = b.kmax
    want_blocks = b.blocks.reshape(b.G, k, b.B).copy()
    want_rows = b.rows.reshape(b.G, k).copy()
    for g in range(b.G):
        slots = np.flatnonzero(want_rows[g] >= k)
        assert len(slots) == b.count[g]
        for j, s in enumerate(slots):
            want_blocks[g, s] = b.out[g, j]
            want_rows[g, s] = b.out_rows[g, j]
    blocks = make_buf("blocks", "out", b.G * k * b.B, mb, rng, b.blocks, unit=k * b.B, device=device)
    blocks.want = want_blocks.reshape(-1)
    rows = make_buf("rows", "out", b.G * k, mr, rng, b.rows, unit=k, device=device)
    rows.want = want_rows.reshape(-1)
    return [blocks, rows]


# ---------------------------------------------------------------- CPU: the checker can fail

def test_checker_catches_damage():
    """The checker passes a correct result (numpy stand-ins holding the Case's own bytes) and fails
    for each kind of damage the GPU tests rely on it to see."""
    b = uniform(28, 4, 256, 37)
    bufs = decode_out_bufs(b, (3, 1, 13, 15, 12), np.random.default_rng(1), device=False)
    by = {x.name: x for x in bufs}

    def good():
        after = {x.name: x.pre.copy() for x in bufs}
        for x in bufs:
            if x.role == "out":
                after[x.name][x.start:x.start + x.nbytes] = x.want
        return after

    check(bufs, good())
    mid = next(g for g in range(10, b.G - 1) if 2 <= b.count[g] < b.emax)  # a middle group with unused slots
    e = int(b.count[mid])
    out, out_rows, count, blocks = by["out"], by["out_rows"], by["out_count"], by["blocks"]

    def flipped_bit(after):
        after["out"][out.start + (mid * b.emax + e - 1) * b.B + 77] ^= 0x10

    def guard_before(after):
        after["out"][out.start - 1] ^= 0xFF

    def guard_after(after):
        after["out"][out.start + out.nbytes] ^= 0x01

    def input_byte(after):
        after["blocks"][blocks.start + (mid * b.kmax + 5) * b.B + 3] ^= 0x80

    def rows_swapped(after):
        p = out_rows.start + mid * b.emax
        r = after["out_rows"]
        assert r[p] != r[p + 1]
        r[p], r[p + 1] = r[p + 1], r[p]

    def count_off_by_one(after):
        after["out_count"][count.start + 4 * mid:count.start + 4 * mid + 4] = \
            np.array([e + 1], "<i4").view(np.uint8)

    for damage, word in ((flipped_bit, "out: output"), (guard_before, "out: guard before"),
                         (guard_after, "out: guard after"), (input_byte, "blocks: read-only input"),
                         (rows_swapped, "out_rows: output"), (count_off_by_one, "out_count: output")):
        after = good()
        damage(after)
        with pytest.raises(AssertionError, match=word):
            check(bufs, after)
    # an unused slot (past the group's count, and the whole of an e = 0 group) must keep its fill
    for g, i in ((mid, b.emax - 1), (3, 0)):
        assert i >= b.count[g]
        after = good()
        after["out"][out.start + (g * b.emax + i) * b.B] ^= 0x01
        with pytest.raises(AssertionError, match="out: output"):
            check(bufs, after)


def test_expectations_cover_every_group():
    """The expected arrays are the oracle's for every group: rebuilt here for one shape straight from
    the oracle calls, independently of Case's bookkeeping."""
    k, m, B, G = 17, 5, 24, 9
    b = uniform(k, m, B, G)
    ora = po.oracle()
    bufs = inplace_bufs(b, (0, 0), np.random.default_rng(2), device=False)
    want_blocks, want_rows = bufs[0].want.reshape(G, k, B), bufs[1].want.reshape(G, k)
    data = b.data.reshape(G, k, B)
    for g in range(G):
        rc, rec = ora.encode(k, m, data[g], B)
        assert rc == 0 and np.array_equal(rec, b.rec[g])
        datas = [x.copy() for x in b.blocks.reshape(G, k, B)[g]]
        rc, new_rows = ora.decode(k, m, datas, [int(r) for r in b.rows.reshape(G, k)[g]], B)
        assert rc == 0 and new_rows == want_rows[g].tolist()
        assert np.array_equal(np.stack(datas), want_blocks[g])
        assert sorted(new_rows) == list(range(k))
        for i, r in enumerate(new_rows):  # a decoded group holds its originals
            assert np.array_equal(datas[i], data[g, r])


# ---------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def sh():
    import torch
    import shorthair_amd
    assert shorthair_amd.cauchy_256_init() == 0
    torch.cuda.init()
    return shorthair_amd


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _ptrs(bufs, *names):
    by = {b.name: b for b in bufs}
    return [by[n].ptr for n in names]


def _ids(params):
    return ["k%d_m%d_B%d_G%d-" % tuple(s[:4]) + "_".join(str(v) for v in t) for s, t in params]


def _product(shapes, tuples):
    """Shape-major: the control tuple of a shape (the first) runs before its misaligned ones."""
    return [(s, t) for s in shapes for t in tuples]


ENC_TUPLES = [(0, 0), (1, 0), (0, 1), (3, 13), (4, 8), (15, 15)]
DEC_TUPLES = [(0, 0, 0, 0, 0), (1, 3, 0, 0, 0), (0, 0, 1, 3, 4), (3, 1, 13, 15, 12), (8, 4, 4, 8, 8),
              (15, 2, 15, 1, 4)]
INPLACE_TUPLES = [(0, 0), (1, 3), (3, 1), (4, 4), (15, 2)]

ENC_SHAPES = [
    (28, 4, 256, 37, "fixed"),     # 16 groups per tile, partial last tile
    (64, 16, 1400, 7, "fixed"),    # groups split across tiles
    (60, 16, 136, 19, "fixed"),    # k below the compiled K: zero-reading steps; shifted tail chunk
    (200, 32, 1400, 5, "fixed"),
    (190, 66, 1336, 4, "fixed"),
    (50, 10, 1000, 7, "tile"),
    (17, 5, 520, 9, "tile"),
    (100, 140, 128, 5, "tile"),    # two row launches
    (20, 5, 64, 11, "generic"),
    (12, 7, 8, 33, "generic"),
    (17, 5, 24, 9, "generic"),     # sub = 3: bytewise loads
    (17, 5, 40, 9, "generic"),     # sub = 5: a one-byte tail word
]
ENC_PARAMS = _product(ENC_SHAPES, ENC_TUPLES)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,mis", ENC_PARAMS, ids=_ids(ENC_PARAMS))
def test_encode_batch_unaligned(sh, shape, mis):
    k, m, B, G, family = shape
    assert sh.path(k, m, B) == family
    b = uniform(k, m, B, G)
    bufs = encode_bufs(b, mis, np.random.default_rng(seed_of(shape[:4], mis)))
    sh.batch_errors()
    assert sh.lib.cauchy_256_encode_batch(k, m, B, G, *_ptrs(bufs, "data", "recovery"), _stream()) == 0
    check(bufs, fetch(bufs))
    assert sh.batch_errors() == 0


DEC_SHAPES = [
    (28, 4, 256, 37, "fixed"),     # stageb_small
    (40, 16, 264, 21, "fixed"),    # stageb_small
    (60, 16, 136, 19, "fixed"),    # stageb_small
    (64, 16, 1400, 7, "fixed"),    # stageb_v2
    (200, 32, 1400, 5, "fixed"),   # stageb_v2
    (190, 66, 1336, 4, "fixed"),   # stageb_v2
    (50, 10, 1000, 7, "tile"),     # stageb_v2 after a tile stage A
    (28, 4, 1400, 9, "fixed"),     # stageb_regs
    (17, 5, 520, 9, "tile"),       # stageb_regs
    (20, 5, 64, 11, "generic"),    # stageb_snip after a generic stage A
    (12, 7, 8, 33, "generic"),     # stageb_snip
    (20, 2, 1400, 5, "tile"),      # m = 2
]
DEC_PARAMS = _product(DEC_SHAPES, DEC_TUPLES)


def _run_decode_out(sh, b, mis, rng, first_mis=None, errors=0):
    """decode_batch_out, or decode_batch_out_var when d_first is placed (first_mis)."""
    bufs = decode_out_bufs(b, mis, rng, first_mis=first_mis)
    ptrs = _ptrs(bufs, "blocks", "rows", "out", "out_rows", "out_count")
    sh.batch_errors()
    if first_mis is None:
        assert sh.lib.cauchy_256_decode_batch_out(b.kmax, b.m, b.B, b.G, *ptrs, _stream()) == 0
    else:
        assert sh.lib.cauchy_256_decode_batch_out_var(b.kmax, b.m, b.B, b.G, _ptrs(bufs, "first")[0], b.total,
                                                      *ptrs, _stream()) == 0
    check(bufs, fetch(bufs))
    assert sh.batch_errors() == errors


@pytest.mark.gpu
@pytest.mark.parametrize("shape,mis", DEC_PARAMS, ids=_ids(DEC_PARAMS))
def test_decode_batch_out_unaligned(sh, shape, mis):
    """count, out_rows[g][:e] and out[g][:e] are the oracle's; the slots from e on keep their fill."""
    k, m, B, G, family = shape
    assert (k, m, B) not in PATHS or PATHS[(k, m, B)] == family
    if family is not None:
        assert sh.path(k, m, B) == family
    b = uniform(k, m, B, G)
    assert (b.count < b.emax).any()  # some unused slots to watch
    _run_decode_out(sh, b, mis, np.random.default_rng(seed_of(shape[:4], mis)))


INPLACE_SHAPES = [(28, 4, 256, 37), (64, 16, 1400, 7), (50, 10, 1000, 7), (17, 5, 520, 9), (20, 5, 64, 11),
                  (12, 7, 8, 33)]
INPLACE_PARAMS = _product(INPLACE_SHAPES, INPLACE_TUPLES)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,mis", INPLACE_PARAMS, ids=_ids(INPLACE_PARAMS))
def test_decode_batch_inplace_unaligned(sh, shape, mis):
    k, m, B, G = shape
    b = uniform(k, m, B, G)
    bufs = inplace_bufs(b, mis, np.random.default_rng(seed_of(shape, mis)))
    sh.batch_errors()
    assert sh.lib.cauchy_256_decode_batch(k, m, B, G, *_ptrs(bufs, "blocks", "rows"), _stream()) == 0
    check(bufs, fetch(bufs))
    assert sh.batch_errors() == 0


MULTI_PARAMS = _product([(28, 4, 128, 8320), (12, 7, 128, 8320)], [DEC_TUPLES[0], DEC_TUPLES[3]])


@pytest.mark.gpu
@pytest.mark.parametrize("shape,mis", MULTI_PARAMS, ids=_ids(MULTI_PARAMS))
def test_multi_group_setups_unaligned(sh, shape, mis):
    """From 8,192 groups on the decode setup runs its multi-group kernels (decode_setup_small for
    m <= 6, decode_setup_cauchy for m >= 7 with emax <= 16), which write out_rows and out_count
    straight into the caller's arrays. A 64-group oracle-built case repeated 130 times."""
    k, m, B, G = shape
    assert G == 64 * 130 and G >= 8192 and (m <= 6 or min(k, m) <= 16)
    b = uniform(k, m, B, 64, rep=130)
    assert b.G == G
    _run_decode_out(sh, b, mis, np.random.default_rng(seed_of(shape, mis)))


VAR_SHAPES = [(28, 4, 256, 37, "fixed"), (50, 10, 1000, 7, "tile"), (20, 5, 64, 11, "generic")]
# (d_first, the call's tuple): the encode and decode tuples without the single-pointer ones
VAR_ENC = [(0, (0, 0)), (4, (3, 13)), (8, (4, 8)), (12, (15, 15))]
VAR_DEC = [(0, DEC_TUPLES[0]), (8, DEC_TUPLES[1]), (12, DEC_TUPLES[2]), (4, DEC_TUPLES[3]), (0, DEC_TUPLES[4]),
           (12, DEC_TUPLES[5])]
VAR_PARAMS = [(s, ("enc",) + t) for s in VAR_SHAPES for t in VAR_ENC] + \
             [(s, ("dec",) + t) for s in VAR_SHAPES for t in VAR_DEC]


def _var_ids(params):
    return ["k%d_m%d_B%d_G%d-" % tuple(s[:4]) + "%s_first%d_" % (c, f) + "_".join(str(v) for v in t)
            for s, (c, f, t) in params]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,call", VAR_PARAMS, ids=_var_ids(VAR_PARAMS))
def test_var_calls_unaligned(sh, shape, call):
    """encode_batch_var and decode_batch_out_var on packed groups of different k: nothing of the
    packed arrays is aligned to begin with, and d_first sits at any multiple of 4."""
    kmax, m, B, G, family = shape
    which, first_mis, mis = call
    assert sh.path(kmax, m, B) == family and first_mis % 4 == 0
    b = nonuniform(kmax, m, B, G)
    rng = np.random.default_rng(seed_of(shape[:4], first_mis, mis))
    if which == "dec":
        _run_decode_out(sh, b, mis, rng, first_mis=first_mis)
        return
    bufs = encode_bufs(b, mis, rng, first_mis=first_mis)
    first, data, rec = _ptrs(bufs, "first", "data", "recovery")
    sh.batch_errors()
    assert sh.lib.cauchy_256_encode_batch_var(kmax, m, B, G, first, b.total, data, rec, _stream()) == 0
    check(bufs, fetch(bufs))
    assert sh.batch_errors() == 0


# ---------------------------------------------------------------- GPU: groups flagged -1

def _with_duplicate_row(b, g):
    """b with group g made malformed (a row listed twice): the header flags it d_out_count[g] = -1,
    counts it, and leaves all of its emax slots untouched."""
    import copy
    assert b.count[g] > 0  # had the group been decoded, its slots would show it
    f = copy.copy(b)
    f.rows, f.count = b.rows.copy(), b.count.copy()
    r = f.rows.reshape(b.G, b.kmax)
    r[g, 1] = r[g, 0]
    f.count[g] = -1
    return f


@functools.lru_cache(maxsize=None)
def flagged(name):
    if name == "fixed":        # one-wave decode_setup, position tables
        return _with_duplicate_row(uniform(28, 4, 256, 37), 1), None
    if name == "generic":      # one-wave decode_setup, per-group stage-A coefficients
        return _with_duplicate_row(uniform(20, 5, 64, 11), 1), None
    if name == "multi_small":  # decode_setup_small
        return _with_duplicate_row(uniform(28, 4, 128, 64, rep=130), 64 * 77 + 1), None
    if name == "multi_cauchy":  # decode_setup_cauchy
        return _with_duplicate_row(uniform(12, 7, 128, 64, rep=130), 64 * 77 + 1), None
    assert name == "var_k1"    # a var-k group of one block: malformed, seen only by the device
    c = Case(28, 4, 256, 12, seed=905, ks=[28, 2, 16, 9, 1, 20, 5, 28, 13, 7, 3, 11])
    assert c.count[4] == -1 and (np.delete(c.count, 4) >= 0).all() and c.count[3] == 0
    return Batch(c, with_data=False), 4


FLAG_PARAMS = [(n, t) for n in ("fixed", "generic", "multi_small", "multi_cauchy", "var_k1")
               for t in (DEC_TUPLES[0], DEC_TUPLES[3])]


@pytest.mark.gpu
@pytest.mark.parametrize("name,mis", FLAG_PARAMS,
                         ids=[n + "-" + "_".join(str(v) for v in t) for n, t in FLAG_PARAMS])
def test_flagged_groups_leave_their_slots_untouched(sh, name, mis):
    """One malformed group among good ones: count -1, one error counted, every byte of its out and
    out_rows slots still the pre-call fill, its neighbours the oracle's."""
    b, first_mis = flagged(name)
    assert (b.count == -1).sum() == 1
    _run_decode_out(sh, b, mis, np.random.default_rng(seed_of(len(name), mis)), first_mis=first_mis, errors=1)


# ---------------------------------------------------------------- GPU: degenerate paths, many groups

DEGENERATE = [("enc", 1, 4, 16), ("enc", 10, 1, 64), ("enc", 10, 1, 13), ("dec", 10, 1, 13), ("dec", 10, 1, 64),
              ("dec", 1, 3, 16)]
DEG_G = 5


@functools.lru_cache(maxsize=None)
def degenerate_case(which, k, m, B):
    """k = 1 / m = 1 groups against the oracle per group. Decode, m = 1: one recovery block per group
    at a different array index per group, and one group with none; k = 1: any row becomes 0."""
    ora = po.oracle()
    rng = np.random.default_rng(seed_of(k, m, B))
    data = rng.integers(0, 256, size=(DEG_G, k, B), dtype=np.uint8)
    rec = np.zeros((DEG_G, m, B), np.uint8)
    for g in range(DEG_G):
        rc, rec[g] = ora.encode(k, m, data[g], B)
        assert rc == 0
    if which == "enc":
        return data, rec
    blocks, rows = data.copy(), np.tile(np.arange(k, dtype=np.uint8), (DEG_G, 1))
    if k == 1:
        for g in range(DEG_G):
            rows[g, 0] = (0, 1, 3, 2, 0)[g]
            if rows[g, 0]:
                blocks[g, 0] = rec[g, rows[g, 0] - 1]
    else:
        where = [0, k - 1, 3, None, 6]  # group 3: no recovery block
        assert len(set(where)) == DEG_G
        for g, j in enumerate(where):
            if j is None:
                continue
            lost = (2 * g + 1) % k
            order = [x for x in range(k) if x != lost]
            order.insert(j, k)  # the recovery block (row k) at array index j
            for i, r in enumerate(order):
                rows[g, i] = r
                blocks[g, i] = rec[g, 0] if r == k else data[g, r]
    want_blocks, want_rows = blocks.copy(), rows.copy()
    for g in range(DEG_G):
        datas = [x.copy() for x in blocks[g]]
        rc, new_rows = ora.decode(k, m, datas, [int(r) for r in rows[g]], B)
        assert rc == 0
        want_blocks[g], want_rows[g] = np.stack(datas), new_rows
    if k > 1:  # the recovery block now holds the lost original; rows stay as they were (m = 1)
        assert np.array_equal(want_rows, rows)
        for g, j in enumerate(where):
            if j is not None:
                assert np.array_equal(want_blocks[g, j], data[g, (2 * g + 1) % k])
        assert np.array_equal(want_blocks[3], blocks[3])
    return blocks, rows, want_blocks, want_rows


DEG_PARAMS = [(c, t) for c in DEGENERATE for t in ((0, 0), (3, 13))]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,mis", DEG_PARAMS,
                         ids=["%s_k%d_m%d_B%d-%d_%d" % (c + t) for c, t in DEG_PARAMS])
def test_degenerate_paths_many_groups(sh, shape, mis):
    """copy_first (k = 1), xor_rows (m = 1, any block_bytes), decode_m1 and decode_k1 with several
    groups in one launch."""
    which, k, m, B = shape
    rng = np.random.default_rng(seed_of(k, m, B, mis))
    if which == "enc":
        data, rec = degenerate_case(which, k, m, B)
        src = make_buf("data", "in", data.size, mis[0], rng, data, unit=k * B)
        dst = make_buf("recovery", "out", rec.size, mis[1], rng, unit=m * B)
        dst.want = rec.reshape(-1)
        bufs = [src, dst]
        assert sh.lib.cauchy_256_encode_batch(k, m, B, DEG_G, src.ptr, dst.ptr, _stream()) == 0
    else:
        blocks, rows, want_blocks, want_rows = degenerate_case(which, k, m, B)
        db = make_buf("blocks", "out", blocks.size, mis[0], rng, blocks, unit=k * B)
        dr = make_buf("rows", "out", rows.size, mis[1], rng, rows, unit=k)
        db.want, dr.want = want_blocks.reshape(-1), want_rows.reshape(-1)
        bufs = [db, dr]
        assert sh.lib.cauchy_256_decode_batch(k, m, B, DEG_G, db.ptr, dr.ptr, _stream()) == 0
    check(bufs, fetch(bufs))
