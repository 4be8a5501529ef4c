"""Every compile-time kernel instantiation against the CPU oracle, at every block geometry class.

The codec ships four kernels per (K, m) of CONFIGS in tools/gen_fixed_kernels.py: enc, dec and
their var-k forms encv, decv (SH_DECL in csrc/fixed_dispatch.cpp). The matrix below is generated
from that list, so a config added to it is covered without an edit here:

  config (K, m)  x  block size class  x  {uniform k = K, uniform k = kmin, var kmax = K}

and every cell runs, at an aligned and at a misaligned set of device pointers, encode, the
out-of-place decode and (uniform cells) the in-place decode, through the harness of
tests/test_batch_alignment.py: every byte of every group against oracle/pyoracle.py run per group,
both guards of every buffer, the read-only inputs, the fill of the unused out / out_rows slots and
cauchy_256_batch_errors() == 0. No expectation comes from the library under test.

Block size classes (COLS = 64 * CW word columns per tile, from the generator's shape(); sub = B / 8,
nq = word columns per sub-block rounded up to 4, shift = 4 * nq - sub = how far the last 16-byte
chunk of a sub-block is moved back):
  B128   sub 16, nq 4, shift 0: most groups per tile
  B136   nq 8, shift 15
  B520   nq 20, shift 15, does not divide COLS, past stageb_small's nq <= 16
  tile   B = 32 * COLS: nq == COLS, shift 0, a group is exactly one tile
  tile+  B = 32 * COLS + 8: nq = COLS + 4, shift 15, a group wider than a tile
Groups: 2 * ceil(COLS / nq) + 3 where nq < COLS (two full tiles, then a partial one that splits a
group), else 3: the smallest batches with a full tile, a partial tile and a straddling group.

Decode patterns are Case's (tests/test_var_batch.py): shuffled array order, groups 0 and 1 at
e = min(k_g, m), group 3 at e = 0, the others random with random recovery-row subsets; the last
group of every cell is made to use recovery rows 0 (the parity row) and m - 1.
"""
import functools
import importlib.util
import os
from collections import namedtuple

import numpy as np
import pytest

from tests.test_batch_alignment import (Batch, _ptrs, _run_decode_out, _stream, check, encode_bufs, fetch,
                                        inplace_bufs, seed_of)
from tests.test_var_batch import Case, _ks

ROOT = os.path.normpath(os.path.join(os.path.dirname(__file__), ".."))


def _gen():
    spec = importlib.util.spec_from_file_location("gen_fixed_kernels", os.path.join(ROOT, "tools", "gen_fixed_kernels.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GEN = _gen()
CONFIGS = [tuple(c) for c in GEN.CONFIGS]
MODES = ("enc", "dec", "encv", "decv")
CLASSES = ("B128", "B136", "B520", "tile", "tile+")
# (encode tuple, decode_out tuple, in-place tuple, d_first): address mod 16 of every buffer
TUPLES = [((0, 0), (0, 0, 0, 0, 0), (0, 0), 0), ((3, 13), (3, 1, 13, 15, 12), (3, 1), 4)]


def cols(K, m):
    """Word columns of one tile of the (K, m) kernels: 64 lanes times CW column waves."""
    return 64 * GEN.shape(K, m)[1]


def geometry(B):
    """fixed_geometry (csrc/geometry.hpp) restated: (sub, nq, shift)."""
    assert B % 8 == 0 and B // 8 >= 16
    sub = B // 8
    nq = ((sub + 3) // 4 + 3) & ~3
    return sub, nq, 4 * nq - sub


def class_B(K, m, cls):
    return {"B128": 128, "B136": 136, "B520": 520, "tile": 32 * cols(K, m), "tile+": 32 * cols(K, m) + 8}[cls]


def class_geometry(K, m, cls):
    """What the class promises: (nq, shift)."""
    c = cols(K, m)
    return {"B128": (4, 0), "B136": (8, 15), "B520": (20, 15), "tile": (c, 0), "tile+": (c + 4, 15)}[cls]


def groups_of(K, m, B):
    nq, c = geometry(B)[1], cols(K, m)
    return 2 * -(-c // nq) + 3 if nq < c else 3


def fixed_k(k, m, B):
    """fixed_kernel_k (csrc/fixed_dispatch.cpp) restated: a kernel compiled for (K, m) codes
    0.6 K <= k <= K (10 k >= 6 K), the smallest fitting K of the same m wins; 0 = none."""
    if B % 8 != 0 or B // 8 < 16 or k < 1:
        return 0
    best = 0
    for K, M in CONFIGS:
        if m == M and k <= K and (k == K or 10 * k >= 6 * K) and (best == 0 or K < best):
            best = K
    return best


def kmin_of(K, m):
    """The smallest k that runs on the (K, m) kernels."""
    return min(k for k in range(1, K + 1) if fixed_k(k, m, 128) == K)


def stageb_route(nq, emax):
    """stageb_route (csrc/stageb_route.hpp) restated for a compile-time stage A (all m residual rows,
    nq % 4 == 0, sub >= 16, emax >= 1): stageb_snip is unreachable."""
    assert nq % 4 == 0 and emax >= 1
    if nq <= 16:
        return "small"
    return "v2" if emax > 8 else "regs"


Cell = namedtuple("Cell", "K m cls B G kind k")  # kind "uni": every k_g = k; "var": kmax = k = K


def build_cells(configs):
    cells = []
    for K, m in configs:
        for cls in CLASSES:
            B = class_B(K, m, cls)
            G = groups_of(K, m, B)
            cells.append(Cell(K, m, cls, B, G, "uni", K))
            cells.append(Cell(K, m, cls, B, G, "uni", kmin_of(K, m)))
            cells.append(Cell(K, m, cls, B, G, "var", K))
    return cells


CELLS = build_cells(CONFIGS)
PARAMS = [(c, t) for c in CELLS for t in range(len(TUPLES))]


def _id(p):
    c, t = p
    return "K%d_m%d-%s_B%d_G%d-%s_k%d-%s" % (c.K, c.m, c.cls, c.B, c.G, c.kind, c.k, ("aligned", "misaligned")[t])


def instantiations(cell):
    """The kernels a cell's calls launch: (K, m, mode)."""
    K = fixed_k(cell.k, cell.m, cell.B)
    return {(K, cell.m, mode) for mode in (("enc", "dec") if cell.kind == "uni" else ("encv", "decv"))}


# ---------------------------------------------------------------- CPU: the matrix itself

KMIN = {(64, 16): 39, (112, 16): 68, (200, 32): 120, (224, 32): 201, (28, 4): 17, (200, 56): 120, (190, 66): 114,
        (216, 40): 130}


def test_matrix_covers_every_instantiation():
    """From the parameter lists alone: every one of the 4 * len(CONFIGS) kernels appears with k = K
    and the uniform ones with k = kmin too, every (config, class) cell exists, and every stage-B
    route a compile-time stage A can reach follows a uniform and a var cell. A config added to the
    generator's list without its cells fails here."""
    configs = [tuple(c) for c in _gen().CONFIGS]
    assert len(configs) == len(set(configs)) >= 8
    cells = {p[0] for p in PARAMS}
    for c in cells:
        assert sum(1 for p in PARAMS if p[0] == c) == len(TUPLES)  # both pointer tuples
    want = {(K, m, mode) for K, m in configs for mode in MODES}
    assert len(want) == 4 * len(configs)
    at_K, at_kmin = set(), set()
    for c in cells:
        assert fixed_k(c.k, c.m, c.B) == c.K, c
        if c.k == c.K:
            at_K |= instantiations(c)
        if c.kind == "uni" and c.k == kmin_of(c.K, c.m):
            at_kmin |= instantiations(c)
    assert at_K == want
    assert at_kmin == {w for w in want if w[2] in ("enc", "dec")}
    for K, m in configs:
        for cls in CLASSES:
            kinds = {(c.kind, c.k) for c in cells if (c.K, c.m, c.cls) == (K, m, cls)}
            assert kinds == {("uni", K), ("uni", kmin_of(K, m)), ("var", K)}, (K, m, cls)
    routes = {"uni": set(), "var": set()}
    for c in cells:
        routes[c.kind].add(stageb_route(geometry(c.B)[1], min(c.k, c.m)))
    reachable = {"small", "v2"} | ({"regs"} if any(m <= 8 for _, m in configs) else set())
    assert routes["uni"] == reachable and routes["var"] == reachable
    # the cells are those of the generator's list, rebuilt here
    assert cells == set(build_cells(configs)) and len(cells) == 3 * len(CLASSES) * len(configs)


def test_block_size_classes_have_their_geometry():
    for K, m in CONFIGS:
        c = cols(K, m)
        assert c % 64 == 0 and c == 64 * GEN.shape(K, m)[1]
        for cls in CLASSES:
            B = class_B(K, m, cls)
            sub, nq, shift = geometry(B)
            assert (nq, shift) == class_geometry(K, m, cls), (K, m, cls)
            assert sub == B // 8 and 0 <= shift < 16 and nq % 4 == 0
            G = groups_of(K, m, B)
            if nq < c:
                # two full tiles and a partial third one
                assert 2 * c < G * nq < 3 * c and G == 2 * -(-c // nq) + 3
            else:
                assert G == 3 and nq in (c, c + 4)
        assert geometry(class_B(K, m, "B520"))[1] > 16 and c % 20 != 0


def test_kmin_is_the_dispatch_rule():
    """kmin restated from fixed_kernel_k, against the library's own answer (host only)."""
    import shorthair_amd as sh
    for K, m in CONFIGS:
        kmin = kmin_of(K, m)
        if (K, m) in KMIN:
            assert kmin == KMIN[(K, m)], (K, m)
        assert 10 * kmin >= 6 * K or kmin == K
        for cls in CLASSES:
            B = class_B(K, m, cls)
            assert sh.path(K, m, B) == "fixed" and sh.path(kmin, m, B) == "fixed", (K, m, B)
            assert sh.path(kmin - 1, m, B) == ("fixed" if fixed_k(kmin - 1, m, B) else "tile"), (K, m, B)
        if not any(M == m and Kx < K for Kx, M in CONFIGS):  # no smaller K of this m takes kmin - 1
            assert fixed_k(kmin - 1, m, 128) == 0


def test_case_options_build_what_they_say():
    """Case's es and force_rows (tests/test_var_batch.py) at a small shape."""
    k, m, B, G = 17, 5, 24, 6
    c = Case(k, m, B, G, seed=11, uniform=True, es=list(range(G)))
    assert c.count.tolist() == list(range(G))
    c = Case(k, m, B, G, seed=12, uniform=True, force_rows={G - 1: (0, m - 1)})
    rows = c.rows.reshape(G, k)[G - 1]
    assert {k, k + m - 1} <= set(int(r) for r in rows) and c.count[G - 1] >= 2 and c.count[3] == 0


# ---------------------------------------------------------------- cases, built once per cell

@functools.lru_cache(maxsize=None)
def cell_case(cell):
    K, m, B, G = cell.K, cell.m, cell.B, cell.G
    seed = seed_of(K, m, B, cell.k, cell.kind == "var") % 1000003
    force = {G - 1: (0, m - 1)}
    if cell.kind == "uni":
        c = Case(cell.k, m, B, G, seed=seed, uniform=True, force_rows=force)
        assert c.ks == [cell.k] * G
    else:
        c = Case(K, m, B, G, seed=seed, force_rows=force)
        assert c.ks == _ks(K, G, seed) and c.ks[0] == 2 and c.ks[1] == K and c.ks[2] < 0.6 * K
    assert c.count[0] == min(c.ks[0], m) and c.count[1] == min(c.ks[1], m) and (G <= 3 or c.count[3] == 0)
    last = c.rows[c.first[G - 1]:c.first[G]]
    assert {c.ks[G - 1], c.ks[G - 1] + m - 1} <= set(int(r) for r in last)
    assert (c.count >= 0).all()
    return Batch(c)


# ---------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def sh():
    import torch
    import shorthair_amd
    assert shorthair_amd.cauchy_256_init() == 0
    torch.cuda.init()
    return shorthair_amd


@pytest.mark.gpu
@pytest.mark.parametrize("cell,t", PARAMS, ids=[_id(p) for p in PARAMS])
def test_matrix_cell(sh, cell, t):
    """encode, decode_batch_out and (uniform) the in-place decode of one cell against the oracle."""
    K, m, B, G, k = cell.K, cell.m, cell.B, cell.G, cell.k
    sub, nq, shift = geometry(B)
    assert (nq, shift) == class_geometry(K, m, cell.cls) and G == groups_of(K, m, B)
    assert sh.path(k, m, B) == "fixed" and fixed_k(k, m, B) == K
    b = cell_case(cell)
    var = cell.kind == "var"
    assert (b.kmax, b.m, b.B, b.G) == (k, m, B, G)
    enc_mis, dec_mis, inplace_mis, first_mis = TUPLES[t]
    first_mis = first_mis if var else None
    rng = np.random.default_rng(seed_of(tuple(cell[:2]) + tuple(cell[3:5]) + (k, var), t))

    bufs = encode_bufs(b, enc_mis, rng, first_mis=first_mis)
    sh.batch_errors()
    if var:
        first, data, rec = _ptrs(bufs, "first", "data", "recovery")
        assert sh.lib.cauchy_256_encode_batch_var(k, m, B, G, first, b.total, data, rec, _stream()) == 0
    else:
        assert sh.lib.cauchy_256_encode_batch(k, m, B, G, *_ptrs(bufs, "data", "recovery"), _stream()) == 0
    check(bufs, fetch(bufs))
    assert sh.batch_errors() == 0
    del bufs

    _run_decode_out(sh, b, dec_mis, rng, first_mis=first_mis)

    if not var:
        bufs = inplace_bufs(b, inplace_mis, rng)
        assert sh.lib.cauchy_256_decode_batch(k, m, B, G, *_ptrs(bufs, "blocks", "rows"), _stream()) == 0
        check(bufs, fetch(bufs))
        assert sh.batch_errors() == 0


ERASURE_PARAMS = [(K, m, B) for K, m in CONFIGS for B in (136, 520)]


@functools.lru_cache(maxsize=None)
def erasure_case(K, m, B):
    emax = min(K, m)
    c = Case(K, m, B, emax + 1, seed=seed_of(K, m, B, 99) % 1000003, uniform=True, es=list(range(emax + 1)))
    assert c.count.tolist() == list(range(emax + 1))
    return Batch(c)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ERASURE_PARAMS, ids=lambda s: "K%d_m%d_B%d" % s)
def test_every_erasure_count(sh, shape):
    """Group g of emax + 1 loses g blocks, in shuffled array order: every residue of e mod 8 of the
    stage-B kernels' eight-at-a-time coefficient reads and every per-e setup (Gauss-Jordan for
    m <= 6, the closed-form inverse above), after stageb_small (B = 136) and after stageb_regs or
    stageb_v2 (B = 520)."""
    K, m, B = shape
    assert sh.path(K, m, B) == "fixed"
    assert stageb_route(geometry(B)[1], min(K, m)) == ("small" if B == 136 else "v2" if min(K, m) > 8 else "regs")
    b = erasure_case(K, m, B)
    _run_decode_out(sh, b, (0, 0, 0, 0, 0), np.random.default_rng(seed_of(shape)))
