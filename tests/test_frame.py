"""Device-resident payload framing (include/shorthair_frame.h: shorthair_frame_batch).

Expected bytes come from the framing rule of Shorthair.cpp:540-557 / :710-735 restated in numpy
below (the rule oracle/packets.py applies per group) and, for the compositions with the var-k
calls, from oracle/packets.py on the CPU oracle -- never from the library under test.
"""
import functools

import numpy as np
import pytest

from oracle import packets as opk
from oracle import pyoracle as po

GAP = 0xA5     # fills every byte of the payload stream that belongs to no payload
CANARY = 0xC3  # around d_blocks
PAD = 4096


def is_malformed(B, payload_bytes, off, ln, raw):
    if raw:
        if ln != B:
            return True
    elif ln < 0 or ln > min(B - 2, 65535):
        return True
    return off < 0 or off + ln > payload_bytes


def frame_rule(B, payload, off, length, raw):
    """blocks[n][B] by the rule; a malformed block is all zeros."""
    n = len(off)
    out = np.zeros((n, B), np.uint8)
    for j in range(n):
        o, ln, r = int(off[j]), int(length[j]), bool(raw[j]) if raw is not None else False
        if is_malformed(B, len(payload), o, ln, r):
            continue
        if r:
            out[j] = payload[o:o + B]
        else:
            out[j, 0], out[j, 1] = ln & 0xFF, ln >> 8
            out[j, 2:2 + ln] = payload[o:o + ln]
    return out


def build_stream(B, total, lead, seed):
    """A payload stream with a `lead`-byte front, gaps between the payloads (all GAP bytes), raw
    blocks at offsets = 3 (mod 8), and the last payload ending exactly at payload_bytes."""
    rng = np.random.default_rng(seed)
    special = [ln for ln in (0, 1, 5, 6, 7, B - 3, B - 2) if 0 <= ln <= B - 2]
    lens = [special[j] if j < len(special) else int(rng.integers(0, B - 1)) for j in range(total)]
    raw = [0] * total
    for j in range(len(special), total):
        if j % 5 == 3:
            raw[j], lens[j] = 1, B
    if total:
        raw[-1], lens[-1] = 0, B - 2
    # stream order differs from block order, but the last block's payload ends the buffer
    order = [int(j) for j in rng.permutation(max(total - 1, 0))] + [total - 1] * (total > 0)
    parts, pos = [np.full(lead, GAP, np.uint8)], lead
    off = np.zeros(total, np.int64)
    for j in order:
        gap = int(rng.integers(0, 10))
        if raw[j]:
            gap += (3 - (pos + gap)) % 8
        parts.append(np.full(gap, GAP, np.uint8))
        pos += gap
        off[j] = pos
        parts.append(rng.integers(0, 256, size=lens[j], dtype=np.uint8))
        pos += lens[j]
    payload = np.concatenate(parts)
    assert all(off[j] % 8 == 3 for j in range(total) if raw[j])
    assert total == 0 or off[-1] + lens[-1] == len(payload)
    return payload, off, np.array(lens, np.int32), np.array(raw, np.uint8)


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
    if a.size == 0:  # a non-null pointer for an empty array
        return torch.zeros(16, dtype=torch.uint8, device="cuda")
    return torch.from_numpy(a).cuda()


def run_frame(sh, B, payload, off, length, raw, misalign=8):
    """Frames on the GPU into a guarded buffer whose base is = misalign (mod 16); checks the canaries
    and that the payload is unchanged; returns (blocks, rc)."""
    import torch
    total = len(off)
    dpay, doff, dlen = _dev(payload), _dev(off), _dev(length)
    draw = _dev(raw) if raw is not None else None
    buf = torch.full((PAD + 16 + total * B + PAD,), CANARY, dtype=torch.uint8, device="cuda")
    start = PAD + (misalign - (buf.data_ptr() + PAD)) % 16
    blocks = buf[start:start + total * B]
    assert (buf.data_ptr() + start) % 16 == misalign
    rc = sh.lib.shorthair_frame_batch(B, total, dpay.data_ptr(), len(payload), doff.data_ptr(), dlen.data_ptr(),
                                      draw.data_ptr() if draw is not None else None, buf.data_ptr() + start,
                                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:start] == CANARY).all() and (got[start + total * B:] == CANARY).all()
    if len(payload):
        assert np.array_equal(dpay.cpu().numpy(), payload)
    return got[start:start + total * B].reshape(total, B), rc, blocks


# ---------------------------------------------------------------- CPU

def test_frame_symbols_exported():
    import shorthair_amd as sh
    for name in ("shorthair_frame_batch", "shorthair_groups_set_framing", "shorthair_groups_traffic"):
        assert name in sh.EXPORTED_SYMBOLS
        assert getattr(sh.lib, name) is not None
    assert callable(sh.frame_batch)


def test_frame_rejects_bad_arguments_without_gpu():
    """Every host-checked argument returns -1 before anything touches the GPU (there is none here)."""
    import shorthair_amd as sh
    f = sh.lib.shorthair_frame_batch
    p = 0x1000  # never dereferenced
    assert f(0, 4, p, 64, p, p, None, p, None) == -1      # block_bytes < 8
    assert f(4, 4, p, 64, p, p, None, p, None) == -1
    assert f(-8, 4, p, 64, p, p, None, p, None) == -1
    assert f(12, 4, p, 64, p, p, None, p, None) == -1     # block_bytes % 8
    assert f(1353, 4, p, 64, p, p, None, p, None) == -1
    assert f(16, -1, p, 64, p, p, None, p, None) == -1    # total_blocks < 0
    assert f(16, 4, p, -1, p, p, None, p, None) == -1     # payload_bytes < 0
    assert f(16, 4, None, 64, p, p, None, p, None) == -1  # null pointers with total_blocks > 0
    assert f(16, 4, p, 64, None, p, None, p, None) == -1
    assert f(16, 4, p, 64, p, None, None, p, None) == -1
    assert f(16, 4, p, 64, p, p, None, None, None) == -1
    for mis in (1, 2, 4, 7, 12):                          # d_blocks not 8-byte aligned
        assert f(16, 4, p, 64, p, p, None, p + mis, None) == -1
        assert f(16, 0, p, 64, p, p, None, p + mis, None) == -1
    assert f(16, 0, None, 0, None, None, None, None, None) == 0  # an empty batch is fine, and no GPU work


def test_rule_restatement_matches_oracle_packets():
    """The numpy rule above frames exactly like oracle/packets.py's tx_group (checked through the
    recovery bytes of a group coded from rule-framed blocks)."""
    ora = po.oracle()
    rng = np.random.default_rng(3)
    packets = [rng.integers(0, 256, size=n, dtype=np.uint8).tobytes() for n in (0, 1, 5, 6, 7, 13, 14, 9)]
    payload = np.frombuffer(b"".join(packets), np.uint8)
    lens = np.array([len(p) for p in packets])
    off = np.concatenate([[0], np.cumsum(lens)[:-1]])
    blocks = frame_rule(16, payload, off, lens, None)
    rc, rec = ora.encode(len(packets), 3, [b for b in blocks], 16)
    assert rc == 0
    assert [bytes([len(packets) + y, len(packets) - 1, 2]) + rec[y].tobytes() for y in range(3)] == \
        opk.tx_group(ora, 3, packets)


# ---------------------------------------------------------------- GPU: kernel against the rule

@pytest.mark.gpu
@pytest.mark.parametrize("B", [8, 16, 24, 136, 1352])
def test_frame_matches_rule(sh, B):
    sh.batch_errors()
    for total in (0, 1, 63, 257):
        for lead in range(16):
            payload, off, length, raw = build_stream(B, total, lead, seed=B * 1000 + total * 16 + lead)
            want = frame_rule(B, payload, off, length, raw)
            got, rc, _ = run_frame(sh, B, payload, off, length, raw, misalign=8)
            assert rc == 0
            bad = [j for j in range(total) if not np.array_equal(got[j], want[j])]
            assert not bad, (total, lead, bad[:4], [(int(off[j]), int(length[j]), int(raw[j])) for j in bad[:4]])
        # a 16-byte-aligned base, and no raw array at all
        payload, off, length, raw = build_stream(B, total, 5, seed=B + total)
        length = np.where(raw != 0, min(B - 2, 3), length).astype(np.int32)
        got, rc, _ = run_frame(sh, B, payload, off, length, None, misalign=0)
        assert rc == 0 and np.array_equal(got, frame_rule(B, payload, off, length, None)), total
    assert sh.batch_errors() == 0


@pytest.mark.gpu
def test_frame_python_binding_on_tensors(sh):
    import torch
    B, total = 136, 63
    payload, off, length, raw = build_stream(B, total, 3, seed=11)
    blocks = torch.zeros((total, B), dtype=torch.uint8, device="cuda")
    assert sh.frame_batch(B, total, _dev(payload), len(payload), _dev(off), _dev(length), _dev(raw), blocks) == 0
    torch.cuda.synchronize()
    assert np.array_equal(blocks.cpu().numpy(), frame_rule(B, payload, off, length, raw))


# ---------------------------------------------------------------- GPU: malformed blocks

@pytest.mark.gpu
def test_frame_malformed_blocks(sh):
    """One malformed block of each kind among good ones: zeros, counted once each, neighbours right."""
    B, total = 136, 40
    payload, off, length, raw = build_stream(B, total, 7, seed=77)
    n = len(payload)
    good_raw = [j for j in range(total) if raw[j]]
    good = [j for j in range(total - 1) if not raw[j]]
    kinds = {
        good[0]: (off[good[0]], -1, 0),                     # len < 0
        good[1]: (off[good[1]], B - 1, 0),                  # len > block_bytes - 2
        good[2]: (-1, 4, 0),                                # span starts before the buffer
        good[3]: (n - 9, 10, 0),                            # span ends one byte past payload_bytes
        good[4]: (1 << 62, 8, 0),                           # far outside (64-bit offsets)
        good[5]: (off[good[5]], 70000, 0),                  # len > 65535
        good_raw[0]: (off[good_raw[0]], B - 8, 1),          # raw block with len != block_bytes
        good_raw[1]: (n - B + 1, B, 1),                     # raw block that ends past payload_bytes
        good_raw[2]: (-3, B, 1),                            # raw block that starts before the buffer
    }
    for j, (o, ln, r) in kinds.items():
        off[j], length[j], raw[j] = o, ln, r
        assert is_malformed(B, n, o, ln, r)
    want = frame_rule(B, payload, off, length, raw)
    assert sum(1 for j in range(total) if not want[j].any() and length[j] != 0) == len(kinds)
    sh.batch_errors()
    got, rc, _ = run_frame(sh, B, payload, off, length, raw)
    assert rc == 0
    assert sh.batch_errors() == len(kinds)
    assert sh.batch_errors() == 0
    for j in range(total):
        if j in kinds:
            assert not got[j].any(), j
        else:
            assert np.array_equal(got[j], want[j]), j


@pytest.mark.gpu
def test_frame_length_limit_of_a_long_block(sh):
    """block_bytes - 2 > 65535: the u16 prefix bounds len (65535 frames, 65536 is malformed)."""
    B = 65544
    rng = np.random.default_rng(5)
    payload = rng.integers(0, 256, size=3 + 65536 + 11, dtype=np.uint8)
    off = np.array([3, 3, 1], np.int64)
    length = np.array([65535, 65536, 9], np.int32)
    want = frame_rule(B, payload, off, length, None)
    assert want[0].any() and not want[1].any()
    sh.batch_errors()
    got, rc, _ = run_frame(sh, B, payload, off, length, None)
    assert rc == 0 and np.array_equal(got, want)
    assert sh.batch_errors() == 1


# ---------------------------------------------------------------- GPU: composition with the var-k calls

COMPOSE = [(28, 4, 136, "fixed"), (20, 10, 136, "tile"), (20, 5, 24, "generic")]


@functools.lru_cache(maxsize=None)
def compose_case(kmax, m, B):
    """Groups of payloads, their oracle recovery packets, and one receive pattern per group with the
    oracle's deliveries."""
    ora = po.oracle()
    rng = np.random.default_rng(kmax * 100 + m)
    ks = [kmax, 2] + [int(v) for v in rng.integers(max(2, (6 * kmax + 9) // 10), kmax + 1, size=4)]
    groups = []
    for k in ks:
        lens = [int(v) for v in rng.integers(0, B - 1, size=k)]
        lens[int(rng.integers(0, k))] = B - 2  # the group's largest payload sets block_bytes
        groups.append([rng.integers(0, 256, size=n, dtype=np.uint8).tobytes() for n in lens])
    recs = [opk.tx_group(ora, m, pk) for pk in groups]
    assert all(len(r[0]) == 3 + B for r in recs)
    rx, want = [], []
    for k, pk, rec in zip(ks, groups, recs):
        e = int(rng.integers(1, min(k, m) + 1))
        lost = set(int(x) for x in rng.choice(k, size=e, replace=False))
        orig = [(i, pk[i]) for i in range(k) if i not in lost]
        orig = [orig[i] for i in rng.permutation(len(orig))]
        got = [rec[int(y)] for y in rng.choice(m, size=e, replace=False)]
        rx.append((orig, got))
        want.append(opk.rx_group(ora, orig, got))
    return ks, groups, recs, rx, want


def _pack(items, rng):
    """items: [(bytes, skip)] -> a buffer with GAP-filled gaps between them; off[] points `skip`
    bytes into each item."""
    parts, off, pos = [], [], 0
    for data, skip in items:
        gap = int(rng.integers(0, 7))
        parts.append(np.full(gap, GAP, np.uint8))
        pos += gap
        off.append(pos + skip)
        parts.append(np.frombuffer(data, np.uint8))
        pos += len(data)
    return np.concatenate(parts), np.array(off, np.int64)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", COMPOSE, ids=lambda s: "k%d_m%d_B%d_%s" % s)
def test_frame_then_var_codec_matches_oracle_packets(sh, shape):
    import torch
    kmax, m, B, family = shape
    assert sh.path(kmax, m, B) == family
    ks, groups, recs, rx, want = compose_case(kmax, m, B)
    G = len(ks)
    rng = np.random.default_rng(9)
    sh.batch_errors()
    # sender: frame -> encode_batch_var
    first = np.concatenate([[0], np.cumsum(ks)]).astype(np.int32)
    total = int(first[-1])
    payload, off = _pack([(p, 0) for pk in groups for p in pk], rng)
    length = np.array([len(p) for pk in groups for p in pk], np.int32)
    blocks = torch.zeros((total, B), dtype=torch.uint8, device="cuda")
    rec = torch.zeros((G, m, B), dtype=torch.uint8, device="cuda")
    assert sh.frame_batch(B, total, _dev(payload), len(payload), _dev(off), _dev(length), None, blocks) == 0
    assert sh.encode_batch_var(kmax, m, B, G, _dev(first), total, blocks, rec) == 0
    got = rec.cpu().numpy()
    for g in range(G):
        wire = [bytes([ks[g] + y, ks[g] - 1, m - 1]) + got[g, y].tobytes() for y in range(m)]
        assert wire == recs[g], g
    # receiver: originals as payloads, recovery packets as they arrived ("[id][k-1][m-1][block]": the
    # block is a raw body 3 bytes into the packet) -> decode_batch_out_var
    items, length, raw, rows = [], [], [], []
    for orig, pkts in rx:
        for oid, p in orig:
            items.append((p, 0))
            length.append(len(p))
            raw.append(0)
            rows.append(oid)
        for pkt in pkts:
            items.append((pkt, 3))
            length.append(B)
            raw.append(1)
            rows.append(pkt[0])
    payload, off = _pack(items, rng)
    blocks = torch.zeros((total, B), dtype=torch.uint8, device="cuda")
    assert sh.frame_batch(B, total, _dev(payload), len(payload), _dev(off), _dev(np.array(length, np.int32)),
                          _dev(np.array(raw, np.uint8)), blocks) == 0
    emax = min(kmax, m)
    out = torch.zeros((G, emax, B), dtype=torch.uint8, device="cuda")
    out_rows = torch.zeros((G, emax), dtype=torch.uint8, device="cuda")
    count = torch.full((G,), -7, dtype=torch.int32, device="cuda")
    assert sh.decode_batch_out_var(kmax, m, B, G, _dev(first), total, blocks, _dev(np.array(rows, np.uint8)), out,
                                   out_rows, count) == 0
    assert sh.batch_errors() == 0
    out, out_rows, count = out.cpu().numpy(), out_rows.cpu().numpy(), count.cpu().numpy()
    for g in range(G):
        e = ks[g] - len(rx[g][0])
        assert count[g] == e, g
        delivered = []
        for i in range(e):  # RecoverGroup :741-756
            ln = int(out[g, i, 0]) | (int(out[g, i, 1]) << 8)
            if ln <= B - 2:
                delivered.append((int(out_rows[g, i]), out[g, i, 2:2 + ln].tobytes()))
        assert delivered == want[g], g
