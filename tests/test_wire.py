"""Device-resident wire framing of recovery blocks (include/shorthair_wire.h: shorthair_wire_emit_batch).

Expected bytes come from the record rule of Shorthair.cpp:598-608 restated in numpy below and, for the
round trip on the device, from oracle/packets.py on the CPU oracle -- never from the library under test.
"""
import numpy as np
import pytest

from oracle import packets as opk
from oracle import pyoracle as po
from tests.test_frame import COMPOSE, GAP, _pack, compose_case, frame_rule

CANARY = 0xC3  # around d_wire
PAD = 4096
INT_MAX = 2**31 - 1


def group_ok(k, first, total, g):
    """var_group's rule (csrc/geometry.hpp); every group of a uniform batch is well formed."""
    if first is None:
        return True
    f0, f1 = int(first[g]), int(first[g + 1])
    return f0 >= 0 and f1 <= total and 2 <= f1 - f0 <= k


def wire_rule(k, m, B, groups, first, total, rec):
    """wire[groups * m][3 + B] by the rule; the records of a malformed group are all zeros."""
    rec = np.asarray(rec, np.uint8).reshape(groups, m, B)
    out = np.zeros((groups, m, 3 + B), np.uint8)
    for g in range(groups):
        if not group_ok(k, first, total, g):
            continue
        kg = k if first is None else int(first[g + 1]) - int(first[g])
        out[g, :, 0] = kg + np.arange(m)
        out[g, :, 1] = kg - 1
        out[g, :, 2] = m - 1
        out[g, :, 3:] = rec[g]
    return out.reshape(groups * m, 3 + B)


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


def run_emit(sh, k, m, B, groups, first, total, rec, wire_mis, rec_mis=0, seed=0):
    """Emits on the GPU into a guarded buffer whose base is = wire_mis (mod 16), from a recovery array
    at = rec_mis (mod 16) with seeded noise behind it; checks the canaries and that the recovery buffer
    is unchanged; returns (wire[groups * m][3 + B], rc)."""
    import torch
    n_in, n_out = groups * m * B, groups * m * (3 + B)
    noise = np.random.default_rng(seed).integers(0, 256, size=16 + n_in + 64, dtype=np.uint8)
    src = torch.from_numpy(noise).cuda()
    s0 = (rec_mis - src.data_ptr()) % 16
    noise[s0:s0 + n_in] = np.asarray(rec, np.uint8).reshape(-1)
    src.copy_(torch.from_numpy(noise))
    assert (src.data_ptr() + s0) % 16 == rec_mis
    dfirst = _dev(np.asarray(first, np.int32)) if first is not None else None
    buf = torch.full((PAD + 16 + n_out + PAD,), CANARY, dtype=torch.uint8, device="cuda")
    start = PAD + (wire_mis - (buf.data_ptr() + PAD)) % 16
    assert (buf.data_ptr() + start) % 16 == wire_mis
    rc = sh.lib.shorthair_wire_emit_batch(k, m, B, groups, dfirst.data_ptr() if dfirst is not None else None,
                                          total, src.data_ptr() + s0, buf.data_ptr() + start,
                                          torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:start] == CANARY).all() and (got[start + n_out:] == CANARY).all(), (B, groups, m, wire_mis)
    assert np.array_equal(src.cpu().numpy(), noise)
    return got[start:start + n_out].reshape(groups * m, 3 + B), rc


# ---------------------------------------------------------------- CPU

def test_wire_symbols_exported():
    import shorthair_amd as sh
    from shorthair_amd import groups as sg
    for name in ("shorthair_wire_emit_batch", "shorthair_groups_set_wire"):
        assert name in sh.EXPORTED_SYMBOLS
        assert getattr(sh.lib, name) is not None
    assert callable(sh.wire_emit_batch) and callable(sg.set_wire)


def test_wire_rejects_bad_arguments_without_gpu():
    """Every host-checked argument returns -1 before anything touches the GPU (there is none here)."""
    import shorthair_amd as sh
    f = sh.lib.shorthair_wire_emit_batch
    p = 0x1000  # never dereferenced
    assert f(200, 32, 1400, 0, None, 0, None, None, None) == 0  # an empty batch is fine, and no GPU work
    assert f(20, 4, 16, 0, p, 0, None, None, None) == 0
    for k in (-1, 0, 1, 256, 300):                                # k outside 2..255
        assert f(k, 1, 16, 4, None, 0, p, p, None) == -1
    for m in (0, -1):                                             # m < 1
        assert f(20, m, 16, 4, None, 0, p, p, None) == -1
    assert f(200, 57, 16, 4, None, 0, p, p, None) == -1           # k + m > 256
    assert f(255, 2, 16, 4, None, 0, p, p, None) == -1
    for B in (0, 4, -8, 12, 1353):                                # block_bytes < 8, or not a multiple of 8
        assert f(20, 4, B, 4, None, 0, p, p, None) == -1
    assert f(20, 4, 16, -1, None, 0, p, p, None) == -1            # groups < 0
    assert f(20, 4, 16, 4, p, -1, p, p, None) == -1               # with d_first: total_blocks < 0
    assert f(20, 4, 16, 4, p, 81, p, p, None) == -1               # total_blocks > groups * k
    for mis in (1, 2, 3):                                         # a misaligned d_first
        assert f(20, 4, 16, 4, p + mis, 40, p, p, None) == -1
    assert f(20, 4, 16, 4, None, 0, None, p, None) == -1          # null pointers with groups > 0
    assert f(20, 4, 16, 4, None, 0, p, None, None) == -1
    for mis in (1, 2, 4, 7, 12):                                  # d_recovery not 8-byte aligned
        assert f(20, 4, 16, 4, None, 0, p + mis, p, None) == -1
        assert f(20, 4, 16, 0, None, 0, p + mis, p, None) == -1
    assert f(20, 32, 16, (INT_MAX // 32) + 1, None, 0, p, p, None) == -1  # groups * m > INT_MAX
    assert f(20, 2, 16, INT_MAX, None, 0, p, p, None) == -1


def test_wire_rule_restatement_matches_oracle_packets():
    """The numpy rule above frames recovery blocks exactly like oracle/packets.py's tx_group."""
    ora = po.oracle()
    rng = np.random.default_rng(3)
    packets = [rng.integers(0, 256, size=n, dtype=np.uint8).tobytes() for n in (0, 1, 5, 6, 7, 13, 14, 9)]
    k, m, B = len(packets), 3, 16
    lens = np.array([len(p) for p in packets])
    off = np.concatenate([[0], np.cumsum(lens)[:-1]])
    blocks = frame_rule(B, np.frombuffer(b"".join(packets), np.uint8), off, lens, None)
    rc, rec = ora.encode(k, m, [b for b in blocks], B)
    assert rc == 0
    wire = wire_rule(k, m, B, 1, None, 0, np.stack(rec))
    assert [w.tobytes() for w in wire] == opk.tx_group(ora, m, packets)
    # the var form of the same group, and a malformed one beside it
    wire = wire_rule(20, m, B, 2, [0, k, k + 1], k + 1, np.stack(list(rec) * 2))
    assert [w.tobytes() for w in wire[:m]] == opk.tx_group(ora, m, packets) and not wire[m:].any()


# ---------------------------------------------------------------- GPU: kernel against the rule

SHAPES = [(1, 1), (1, 2), (3, 5), (7, 32), (67, 4)]  # runs from 11 bytes (B = 8) up to several workgroups


@pytest.mark.gpu
@pytest.mark.parametrize("B", [8, 16, 24, 136, 1352])
def test_emit_matches_rule(sh, B):
    k = 200
    for groups, m in SHAPES:
        rec = np.random.default_rng(B * 100 + groups).integers(0, 256, size=(groups, m, B), dtype=np.uint8)
        want = wire_rule(k, m, B, groups, None, 0, rec)
        for wire_mis in range(16):
            for rec_mis in (0, 8):
                got, rc = run_emit(sh, k, m, B, groups, None, 0, rec, wire_mis, rec_mis, seed=wire_mis)
                assert rc == 0
                bad = np.flatnonzero((got != want).any(axis=1))
                assert not len(bad), (groups, m, wire_mis, rec_mis, bad[:4])


@pytest.mark.gpu
def test_emit_long_block(sh):
    """3 + block_bytes past any multiply-by-reciprocal range."""
    B, groups, m, k = 65544, 1, 2, 100
    rec = np.random.default_rng(6).integers(0, 256, size=(groups, m, B), dtype=np.uint8)
    want = wire_rule(k, m, B, groups, None, 0, rec)
    for wire_mis in (0, 5, 8, 15):
        got, rc = run_emit(sh, k, m, B, groups, None, 0, rec, wire_mis, 8)
        assert rc == 0 and np.array_equal(got, want), wire_mis
    first = [0, 77]
    got, rc = run_emit(sh, k, m, B, groups, first, 77, rec, 3)
    assert rc == 0 and np.array_equal(got, wire_rule(k, m, B, groups, first, 77, rec))


@pytest.mark.gpu
@pytest.mark.parametrize("B,m", [(8, 3), (24, 1), (136, 5), (1352, 4)])
def test_emit_var_k_and_malformed_groups(sh, B, m):
    """kmax = 20, k_g mixed in 2..20, one malformed group of each kind: their records are zeros, every
    other record is right, and nothing is counted."""
    kmax = 20
    rng = np.random.default_rng(B + m)
    ks = [20, 2, 7, 1, 13, 21, 5, 20] + [int(v) for v in rng.integers(2, 21, size=17)]
    groups = len(ks)
    first = np.concatenate([[0], np.cumsum(ks)]).astype(np.int32)
    total = int(first[-1]) - 1   # the last group's span ends one block past total_blocks
    first[0] = -1                # group 0 starts before the array
    bad = [g for g in range(groups) if not group_ok(kmax, first, total, g)]
    assert bad == [0, 3, 5, groups - 1] and total <= groups * kmax
    rec = rng.integers(1, 256, size=(groups, m, B), dtype=np.uint8)
    want = wire_rule(kmax, m, B, groups, first, total, rec)
    assert all(not want[g * m:(g + 1) * m].any() for g in bad)
    assert sh.batch_errors() >= 0
    assert sh.batch_errors() == 0
    for wire_mis in (0, 1, 6, 8, 11, 15):
        got, rc = run_emit(sh, kmax, m, B, groups, first, total, rec, wire_mis, 8 * (wire_mis & 1))
        assert rc == 0
        wrong = np.flatnonzero((got != want).any(axis=1))
        assert not len(wrong), (wire_mis, wrong[:4])
    assert sh.batch_errors() == 0  # emit counts nothing: the encode call before it did


@pytest.mark.gpu
def test_emit_python_binding_on_tensors(sh):
    import torch
    k, m, B, groups = 28, 4, 136, 9
    rng = np.random.default_rng(12)
    rec = rng.integers(0, 256, size=(groups, m, B), dtype=np.uint8)
    wire = torch.zeros((groups * m, 3 + B), dtype=torch.uint8, device="cuda")
    assert sh.wire_emit_batch(k, m, B, groups, None, 0, _dev(rec), wire) == 0
    torch.cuda.synchronize()
    assert np.array_equal(wire.cpu().numpy(), wire_rule(k, m, B, groups, None, 0, rec))
    ks = [int(v) for v in rng.integers(2, k + 1, size=groups)]
    first = np.concatenate([[0], np.cumsum(ks)]).astype(np.int32)
    wire.zero_()
    assert sh.wire_emit_batch(k, m, B, groups, _dev(first), int(first[-1]), _dev(rec), wire) == 0
    torch.cuda.synchronize()
    assert np.array_equal(wire.cpu().numpy(), wire_rule(k, m, B, groups, first, int(first[-1]), rec))
    assert sh.wire_emit_batch(k, m, B + 1, groups, None, 0, _dev(rec), wire) == -1


# ---------------------------------------------------------------- GPU: round trip on the device

@pytest.mark.gpu
@pytest.mark.parametrize("shape", COMPOSE, ids=lambda s: "k%d_m%d_B%d_%s" % s)
def test_round_trip_on_the_device(sh, shape):
    """frame_batch -> encode_batch_var -> wire_emit_batch gives tx_group's packets; the receiver's
    frame_batch reads them in place (raw blocks at record offset + 3) beside the surviving originals'
    payloads, and decode_batch_out_var -> unframe_batch delivers rx_group's lists."""
    import torch
    kmax, m, B, family = shape
    assert sh.path(kmax, m, B) == family
    ks, groups, recs, rx, want = compose_case(kmax, m, B)
    G, S = len(ks), 3 + B
    rng = np.random.default_rng(14)
    sh.batch_errors()
    first = np.concatenate([[0], np.cumsum(ks)]).astype(np.int32)
    total = int(first[-1])
    dfirst = _dev(first)
    # one device buffer: the surviving originals' payloads (gaps between them), then the wire region
    front, orig_off = _pack([(p, 0) for orig, _ in rx for _, p in orig], rng)
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
    got = ring.cpu().numpy()
    assert np.array_equal(got[:len(front)], front) and (got[len(front):wire_off] == GAP).all()
    assert got[wire_off:].tobytes() == b"".join(pkt for r in recs for pkt in r)
    # receiver: rows and first[] come from the host, the block bytes never leave the device
    off, length, raw, rows, o = [], [], [], [], 0
    for g, (orig, pkts) in enumerate(rx):
        for oid, p in orig:
            off.append(int(orig_off[o]))
            o += 1
            length.append(len(p))
            raw.append(0)
            rows.append(oid)
        for pkt in pkts:
            y = pkt[0] - ks[g]
            off.append(wire_off + (g * m + y) * S + 3)
            length.append(B)
            raw.append(1)
            rows.append(pkt[0])
    blocks = torch.zeros((total, B), dtype=torch.uint8, device="cuda")
    assert sh.frame_batch(B, total, ring, ring.numel(), _dev(np.array(off, np.int64)),
                          _dev(np.array(length, np.int32)), _dev(np.array(raw, np.uint8)), blocks) == 0
    emax = min(kmax, m)
    slots = G * emax
    out = torch.full((G, emax, B), 0x77, dtype=torch.uint8, device="cuda")
    out_rows = torch.zeros((G, emax), dtype=torch.uint8, device="cuda")
    count = torch.full((G,), -7, dtype=torch.int32, device="cuda")
    assert sh.decode_batch_out_var(kmax, m, B, G, dfirst, total, blocks, _dev(np.array(rows, np.uint8)), out,
                                   out_rows, count) == 0
    cap = slots * (B - 2)
    pay = torch.full((cap,), CANARY, dtype=torch.uint8, device="cuda")
    doff = torch.zeros(slots + 1, dtype=torch.int64, device="cuda")
    dlen = torch.zeros(slots, dtype=torch.int32, device="cuda")
    scratch = torch.zeros(sh.unframe_scratch_bytes(G, emax), dtype=torch.uint8, device="cuda")
    assert sh.unframe_batch(B, G, emax, emax, out, count, pay, cap, doff, dlen, scratch) == 0
    assert sh.batch_errors() == 0
    pay, doff, dlen, out_rows = pay.cpu().numpy(), doff.cpu().numpy(), dlen.cpu().numpy(), out_rows.cpu().numpy()
    for g in range(G):
        delivered = [(int(out_rows[g, i]), pay[doff[s]:doff[s] + dlen[s]].tobytes())
                     for i in range(emax) for s in [g * emax + i] if dlen[s] >= 0]
        assert delivered == want[g], g
