"""Blocks whose span passes 2^31 (include/cauchy_256_batch.h, "Large blocks").

The compile-time and the tile kernels address a workgroup's groups through one buffer descriptor of
at most 0x7FFFFFFF bytes and 32-bit offsets (csrc/stagea_route.hpp states the three formulas). A
shape whose offsets cannot stay below 2^31 must run the generic kernels, whose addresses are 64-bit
pointers, and cauchy_256_batch_path must say so. Required of every admitted shape: the bytes are the
oracle's, or the call returns -1 before anything is enqueued. This pull request adds no such -1.

CPU: the bound restated and path() on both sides of it; the route function compiled alone; and the
sampling identity the GPU checks lean on, on the oracle alone.

Sampling identity. The code acts on byte position j of the eight sub-blocks of a block
independently of every other position. So for a set J of positions inside a sub-block, gathering
bytes a * sub + j (a = 0..7, j in J) of every block gives an instance with blocks of 8 |J| bytes,
and its encode and decode are the same gather of the full result, rows included.

GPU: the smallest shapes that cross each bound, with seeded torch.randint data made on the device:
  G = 2, k * B ~ 1.5 * 2^30   a tile straddling two groups passes 2^31 from the first group's start
  G = 1, k * B ~ 1.25 * 2^31  one group passes 2^31
  G = 1, k * B ~ 1.1 * 2^32   the step term x * B passes 2^32
each at a compile-time shape, (28, 4), and a tile shape, (50, 10), and
  G = 1, m * B ~ 1.25 * 2^31  the output side, at the tile shape (8, 20) with m > k.
Per case: encode, then decode_batch_out with e = min(k, m) in shuffled order. (a) On the device every
recovered block equals the erased original over all its bytes. (b) On the host, through the sampling
identity, the recovery blocks, out, out_rows and count equal the oracle's at the first and last 16
positions of a sub-block, 32 seeded random ones, and every position that some (group, block,
sub-block) puts within 16 bytes of a multiple of 2^31 in the data, recovery, blocks or out buffer.
"""
import os
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po

ROOT = os.path.normpath(os.path.join(os.path.dirname(__file__), ".."))
LIMIT = 0x7FFFFFFF


# ---------------------------------------------------------------- the bound, restated

def fixed_nq(B):
    return ((B // 8 + 3) // 4 + 3) & ~3


def span_fits(k, m, B):
    """stagea_span_fits (csrc/stagea_route.hpp): a tile of at most 512 columns overlaps at most
    n = 511 / nq + 2 groups, each of max(k, m) * B bytes on its wider side."""
    if B % 8 != 0 or B // 8 < 16:
        return True
    return (511 // fixed_nq(B) + 2) * max(k, m) * B <= LIMIT


def last_fitting_B(k, m):
    B = LIMIT // (2 * max(k, m)) // 8 * 8
    assert fixed_nq(B) >= 512 and span_fits(k, m, B) and not span_fits(k, m, B + 8)
    return B


# (k, m, family below the bound): a compile-time shape, a tile shape, a tile shape with m > k
SIDES = [(28, 4, "fixed"), (50, 10, "tile"), (8, 20, "tile"), (200, 56, "fixed"), (130, 40, "fixed"), (2, 254, "tile")]


def test_path_on_both_sides_of_the_bound():
    import shorthair_amd as sh
    for k, m, family in SIDES:
        B = last_fitting_B(k, m)
        assert 2 * max(k, m) * B <= LIMIT < 2 * max(k, m) * (B + 8)
        assert sh.path(k, m, B) == family, (k, m, B)
        assert sh.path(k, m, B - 8) == family, (k, m, B)
        assert sh.path(k, m, B + 8) == "generic", (k, m, B)
        assert sh.path(k, m, 2 * B) == "generic" and sh.path(k, m, 4 * B + 8) == "generic", (k, m, B)
    # input side and output side are the same bound on the wider of the two
    assert last_fitting_B(8, 20) == last_fitting_B(20, 8) == LIMIT // 40 // 8 * 8
    # blocks whose sub-block has fewer than 512 columns never reach it, at any k and m
    for B in (128, 1400, 4096, 16256):
        assert fixed_nq(B) < 512
        for k, m in ((255, 1), (1, 255), (128, 128), (200, 56)):
            assert span_fits(k, m, B)
    assert fixed_nq(16264) == 512
    for k, m, family in ((200, 56, "fixed"), (28, 4, "fixed"), (50, 10, "tile")):
        assert sh.path(k, m, 16256) == family and sh.path(k, m, 65536) == family
    # the GPU cases below are past it
    for k, m, B, G, _ in BIG:
        assert not span_fits(k, m, B) and sh.path(k, m, B) == "generic", (k, m, B)


def test_span_route_compiled_alone(tmp_path):
    """stagea_span_fits and stagea_route's `fits` input from csrc/stagea_route.hpp in a stand-alone
    host program: the bound agrees with its restatement here on both sides, and a shape that does not
    fit is Generic and unsliced, with round4(k) position tables, whatever the other inputs say."""
    shapes = []
    for k, m, _ in SIDES:
        B = last_fitting_B(k, m)
        shapes += [(k, m, B), (k, m, B + 8)]
    shapes += [(255, 1, 16256), (255, 1, 16264), (128, 128, 8388600), (128, 128, 8388608), (28, 4, 120), (28, 4, 100)]
    shapes += [s[:3] for s in BIG]
    rows = ", ".join("{%d, %d, %d}" % s for s in shapes)
    src = tmp_path / "span.cpp"
    src.write_text(r'''
#include "stagea_route.hpp"
#include <cstdio>
int main() {
    const int shapes[][3] = {%s};
    for (const auto &s : shapes) std::putchar(sh::stagea_span_fits(s[0], s[1], s[2]) ? '1' : '0');
    std::putchar('\n');
    for (int kfix : {0, 28, 64})
        for (int tile = 0; tile < 2; ++tile)
            for (int dec = 0; dec < 2; ++dec)
                for (int slices : {1, 8}) {
                    const sh::StageAPlan p = sh::stagea_route(28, kfix, tile != 0, dec != 0, slices, false);
                    if (p.route != sh::StageARoute::Generic || p.sliced || p.kp != 28) return 1;
                    const sh::StageAPlan q = sh::stagea_route(28, kfix, tile != 0, dec != 0, slices, true);
                    const sh::StageAPlan r = sh::stagea_route(28, kfix, tile != 0, dec != 0, slices);
                    if (q.route != r.route || q.sliced != r.sliced || q.kp != r.kp) return 2;
                }
    return 0;
}
''' % rows)
    exe = tmp_path / "span"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-std=c++17", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'shorthair_amd', 'csrc')}",
                    str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True, timeout=60).stdout
    assert out.strip() == "".join("1" if span_fits(*s) else "0" for s in shapes)
    assert out.strip().startswith("10" * len(SIDES))


# ---------------------------------------------------------------- the sampling identity

def gather(x, sub, J):
    """Bytes a * sub + j (a = 0..7, j in J) of every block: x [..., 8 * sub] -> [..., 8 * len(J)]."""
    x = np.asarray(x)
    assert x.shape[-1] == 8 * sub
    return np.ascontiguousarray(x.reshape(x.shape[:-1] + (8, sub))[..., J]).reshape(x.shape[:-1] + (8 * len(J),))


def pattern(k, m, e, rng):
    """A decode pattern with e erasures in shuffled array order: (rows[k], lost ascending)."""
    lost = np.sort(rng.choice(k, size=e, replace=False))
    ys = np.sort(rng.choice(m, size=e, replace=False))
    rows = np.concatenate([np.setdiff1d(np.arange(k), lost), k + ys])[rng.permutation(k)]
    return [int(r) for r in rows], [int(x) for x in lost]


def oracle_decode(ora, k, m, blocks, rows, B):
    """(new rows, blocks after the in-place decode)."""
    datas = [np.ascontiguousarray(b).copy() for b in blocks]
    rc, new_rows = ora.decode(k, m, datas, rows, B)
    assert rc == 0
    return new_rows, np.stack(datas)


@pytest.mark.parametrize("k,m,B", [(28, 4, 256), (200, 56, 1352), (17, 5, 520), (12, 7, 64), (224, 32, 4104)])
def test_sampling_identity_on_the_oracle(k, m, B):
    ora = po.oracle()
    rng = np.random.default_rng(k * 1000 + m)
    sub = B // 8
    data = rng.integers(0, 256, size=(k, B), dtype=np.uint8)
    rc, rec = ora.encode(k, m, data, B)
    assert rc == 0
    e = min(k, m)
    rows, lost = pattern(k, m, e, rng)
    blocks = np.stack([data[r] if r < k else rec[r - k] for r in rows])
    new_rows, after = oracle_decode(ora, k, m, blocks, rows, B)
    assert sorted(new_rows) == list(range(k))
    for J in ([0], [sub - 1], sorted({0, sub - 1} | set(int(j) for j in rng.choice(sub, size=min(sub, 5), replace=False)))):
        Bs = 8 * len(J)
        rc, rec_s = ora.encode(k, m, gather(data, sub, J), Bs)
        assert rc == 0 and np.array_equal(rec_s, gather(rec, sub, J)), J
        rows_s, after_s = oracle_decode(ora, k, m, gather(blocks, sub, J), rows, Bs)
        assert rows_s == new_rows and np.array_equal(after_s, gather(after, sub, J)), J


# ---------------------------------------------------------------- GPU

# (k, m, B, G, what crosses)
BIG = [
    (28, 4, 57521880, 2, "two groups in one tile: k * B = 1.5 * 2^30"),
    (28, 4, 95869800, 1, "one group: k * B = 1.25 * 2^31"),
    (28, 4, 168730856, 1, "the step term: k * B = 1.1 * 2^32"),
    (50, 10, 32212248, 2, "two groups in one tile: k * B = 1.5 * 2^30"),
    (50, 10, 53687088, 1, "one group: k * B = 1.25 * 2^31"),
    (50, 10, 94489288, 1, "the step term: k * B = 1.1 * 2^32"),
    (8, 20, 134217720, 1, "the output side: m * B = 1.25 * 2^31"),
]
TARGETS = [1.5 * 2 ** 30, 1.25 * 2 ** 31, 1.1 * 2 ** 32, 1.5 * 2 ** 30, 1.25 * 2 ** 31, 1.1 * 2 ** 32, 1.25 * 2 ** 31]


def crossings(n_blocks, B, G):
    """Positions j inside a sub-block that some byte within 16 bytes of a multiple of 2^31 of a
    [G][n_blocks][B] buffer has, and the number of multiples inside the buffer."""
    sub, total = B // 8, G * n_blocks * B
    js, n = set(), 0
    for M in range(2 ** 31, total, 2 ** 31):
        n += 1
        ps = [p for p in range(M - 16, M + 16) if 0 <= p < total]
        assert M - 1 in ps and M in ps  # one position on each side at the least
        js |= {(p % B) % sub for p in ps}
        assert ((M - 1) % B) % sub in js and (M % B) % sub in js
    return js, n


def positions(k, m, B, G, rng):
    sub = B // 8
    J = set(range(16)) | set(range(sub - 16, sub)) | set(int(j) for j in rng.choice(sub, size=32, replace=False))
    ncross = 0
    for n_blocks in (k, m, min(k, m)):  # data and blocks, recovery, out
        js, n = crossings(n_blocks, B, G)
        J |= js
        ncross += n
    return sorted(J), ncross


def test_big_shapes_are_what_they_claim():
    for (k, m, B, G, _), target in zip(BIG, TARGETS):
        assert B % 8 == 0 and abs(max(k, m) * B - target) <= 8 * max(k, m)
        assert (B // 8) % 4 != 0  # a sub-block with a short last word
        J, ncross = positions(k, m, B, G, np.random.default_rng(1))
        assert ncross >= 1 and 32 <= len(J) <= 64 + 32 * ncross and J[0] == 0 and J[-1] == B // 8 - 1
    assert 2 * 28 * 57521880 > LIMIT > 28 * 57521880          # only with two groups
    assert 2 ** 32 > 28 * 95869800 > 2 ** 31                   # one group, every x * B below 2^32
    assert 28 * 168730856 > 2 ** 32 and 50 * 94489288 > 2 ** 32
    assert 20 * 134217720 > 2 ** 31 > 8 * 134217720            # the output side alone


@pytest.fixture(scope="module")
def sh():
    import torch
    import shorthair_amd
    assert shorthair_amd.cauchy_256_init() == 0
    torch.cuda.init()
    return shorthair_amd


def sample(t, sub, J):
    """gather() of a device tensor [..., 8 * sub], on the host."""
    import torch
    idx = torch.as_tensor(J, device=t.device)
    return t.reshape(t.shape[:-1] + (8, sub)).index_select(-1, idx).reshape(t.shape[:-1] + (8 * len(J),)).cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("case", BIG, ids=lambda c: "k%d_m%d_B%d_G%d" % c[:4])
def test_big_blocks_match_the_oracle(sh, case):
    import torch
    k, m, B, G, _ = case
    assert sh.path(k, m, B) == "generic"
    sub, e = B // 8, min(k, m)
    rng = np.random.default_rng(k * 7 + m + B)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(k * 1000003 + B)
    data = torch.empty((G, k, B), dtype=torch.uint8, device="cuda")
    for g in range(G):
        for x in range(k):
            data[g, x] = torch.randint(0, 256, (B,), dtype=torch.uint8, device="cuda", generator=gen)
    rec = torch.full((G, m, B), 0x5A, dtype=torch.uint8, device="cuda")
    sh.batch_errors()
    assert sh.encode_batch(k, m, B, G, data, rec) == 0
    torch.cuda.synchronize()

    pats = [pattern(k, m, e, rng) for _ in range(G)]
    rows = np.array([p[0] for p in pats], np.uint8)
    assert len({tuple(r) for r in rows.tolist()}) == G and not any(p[0] == sorted(p[0]) for p in pats)
    blocks = torch.empty((G, k, B), dtype=torch.uint8, device="cuda")
    for g in range(G):
        for i, r in enumerate(pats[g][0]):
            blocks[g, i] = data[g, r] if r < k else rec[g, r - k]
    out = torch.full((G, e, B), 0xA5, dtype=torch.uint8, device="cuda")
    out_rows = torch.full((G, e), 0xEE, dtype=torch.uint8, device="cuda")
    count = torch.full((G,), -7, dtype=torch.int32, device="cuda")
    assert sh.decode_batch_out(k, m, B, G, blocks, torch.from_numpy(rows).cuda(), out, out_rows, count) == 0
    assert sh.batch_errors() == 0

    # (a) every recovered block is the erased original, over all its bytes
    assert count.cpu().tolist() == [e] * G
    assert out_rows.cpu().tolist() == [p[1] for p in pats]
    for g in range(G):
        for i, x in enumerate(pats[g][1]):
            assert torch.equal(out[g, i], data[g, x]), (g, i, x)

    # (b) the oracle at the sampled positions
    J, ncross = positions(k, m, B, G, rng)
    assert ncross >= 1
    Bs = 8 * len(J)
    ora = po.oracle()
    data_s, rec_s, blocks_s, out_s = (sample(t, sub, J) for t in (data, rec, blocks, out))
    for g in range(G):
        rc, want = ora.encode(k, m, data_s[g], Bs)
        assert rc == 0
        bad = np.argwhere(rec_s[g] != want)
        assert bad.size == 0, "recovery: group %d row %d sub-block %d position %d" % (
            g, bad[0][0], bad[0][1] // len(J), J[bad[0][1] % len(J)])
        new_rows, after = oracle_decode(ora, k, m, blocks_s[g], pats[g][0], Bs)
        slots = [i for i, r in enumerate(pats[g][0]) if r >= k]
        assert [new_rows[i] for i in slots] == pats[g][1]
        bad = np.argwhere(out_s[g] != after[slots])
        assert bad.size == 0, "out: group %d slot %d sub-block %d position %d" % (
            g, bad[0][0], bad[0][1] // len(J), J[bad[0][1] % len(J)])
