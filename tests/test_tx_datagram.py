"""shorthair_tx_datagram_batch (include/shorthair_tx.h): datagrams in send order, written on the GPU.

Expected values come from `tx_rule` below, a datagram-by-datagram restatement of the header's rule, and for
the large cases from `tx_rule_np`, a vectorised form that is first proved equal to the sequential one on the
small cases. `tx_rule` itself is pinned to the reference by tests/golden/tx_datagrams.npz, the server's side of
a run of the reference's protocol layer (tools/capture_tx_datagrams.py). Recovery bytes come from
oracle/packets.py on the CPU oracle; nothing comes from the library under test."""
import functools
import os

import numpy as np
import pytest

from oracle import packets as opk
from oracle import pyoracle as po
from tests.test_rx_group import _dev, dev_bucket, dev_group, expand, slot_records
from tests.test_rx_list import CANARY, Guarded

TILE = 256            # SHORTHAIR_TX_TILE
TILE_PASS = 1024      # SHORTHAIR_TX_TILE_PASS
MAX_BLOCK = 65544     # SHORTHAIR_TX_MAX_BLOCK_BYTES
MAX_DATAGRAM = 65550  # SHORTHAIR_TX_MAX_DATAGRAM_BYTES
INCLUDE = os.path.join(os.path.dirname(__file__), "..", "include")
FIXTURE = os.path.join(os.path.dirname(__file__), "golden", "tx_datagrams.npz")
DESC = np.dtype([("rec_off", "<i8"), ("m", "<i4"), ("block_bytes", "<i4")])
HOLE = -1


def orig(g, x):
    return (g << 9) | x


def recov(g, y):
    return (g << 9) | 256 | y


def roundup(x, a):
    return (x + a - 1) // a * a


# ---------------------------------------------------------------- the rule

def case(sched, first, payload, off, ln, recovery=None, group=None, m=0, B=0, pong_at=(), pong_val=(), state=(0, 0),
         advance=0, align=1, ring_bytes=None, payload_bytes=None, recovery_bytes=None, total=None, groups=None):
    """The arguments of one call, as host arrays."""
    c = dict(sched=np.asarray(sched, np.int32), first=np.asarray(first, np.int32),
             payload=np.asarray(payload, np.uint8), off=np.asarray(off, np.int64), ln=np.asarray(ln, np.int32),
             recovery=None if recovery is None else np.asarray(recovery, np.uint8),
             group=None if group is None else np.asarray(group, DESC), m=m, B=B,
             pong_at=np.asarray(pong_at, np.int32), pong_val=np.asarray(pong_val, np.uint32).reshape(-1),
             state=np.asarray(state, np.int32), advance=advance, align=align)
    c["groups"] = len(c["first"]) - 1 if groups is None else groups
    c["total"] = len(c["off"]) if total is None else total
    c["payload_bytes"] = len(c["payload"]) if payload_bytes is None else payload_bytes
    c["recovery_bytes"] = (0 if c["recovery"] is None else len(c["recovery"])) if recovery_bytes is None else recovery_bytes
    c["ring_bytes"] = ring_bytes
    return c


def one_datagram(c, i):
    """Steps 1 to 7 of the header for datagram i: (class, bytes). Malformed: (-1, b"")."""
    BAD = (-1, b"")
    e = int(c["sched"][i])
    seq = (int(c["state"][0]) + i) & 0xffff
    head = bytes([seq & 255, seq >> 8])
    q = [t for t, at in enumerate(c["pong_at"]) if at == i]
    pong = b""
    if q:
        seen, total = int(c["pong_val"][2 * q[0]]), int(c["pong_val"][2 * q[0] + 1])
        pong = bytes([0x81]) + seen.to_bytes(4, "little") + total.to_bytes(4, "little")
    if e == -1:  # 1
        return (11, head + pong) if pong else (3, b"")
    if e < -1:  # 2
        return BAD
    g, x = e >> 9, e & 511
    if g >= c["groups"]:
        return BAD
    f0, f1 = int(c["first"][g]), int(c["first"][g + 1])  # 3
    k = f1 - f0
    if f0 < 0 or f1 > c["total"] or k < 1 or k > 255:
        return BAD
    g7 = (int(c["state"][1]) + g) & 0x7f

    def payload(j):
        o, n = int(c["off"][j]), int(c["ln"][j])
        if n < 0 or n > 65535 or o < 0 or o + n > c["payload_bytes"]:
            return None
        return c["payload"][o:o + n].tobytes()

    if x < 256:  # 4
        if x >= k:
            return BAD
        p = payload(f0 + x)
        if p is None:
            return BAD
        return (8 if pong else 0, head + pong + bytes([g7, x, x]) + p)
    y = x - 256  # 5
    if pong:
        return BAD
    if c["group"] is not None:
        rec_off, m, B = (int(v) for v in c["group"][g])
    else:
        rec_off, m, B = g * c["m"] * c["B"], c["m"], c["B"]
    if m < 1 or y >= m or k + m > 256:
        return BAD
    if k == 1:  # 6
        p = payload(f0)
        return BAD if p is None else (2, head + bytes([g7, 1, 0]) + p)
    if B < 8 or B % 8 or B > MAX_BLOCK or rec_off < 0 or rec_off % 8 or rec_off + m * B > c["recovery_bytes"]:  # 7
        return BAD
    at = rec_off + y * B
    return (1, head + bytes([g7, k + y, k - 1, m - 1]) + c["recovery"][at:at + B].tobytes())


def place(c, cls, length):
    """Placement and the other outputs from the per-datagram classes and lengths (arrays)."""
    n = len(cls)
    cls, length = cls.astype(np.int32), length.astype(np.int64)
    step = (length + c["align"] - 1) // c["align"] * c["align"]
    dg_off = np.zeros(n + 1, np.int64)
    np.cumsum(step, out=dg_off[1:])
    ring_bytes = int(dg_off[n]) if c["ring_bytes"] is None else c["ring_bytes"]
    over = (length > 0) & (dg_off[:n] + length > ring_bytes)
    malformed = int((cls == -1).sum())
    cls = np.where(over, -2, cls).astype(np.int32)
    length = np.where(over, 0, length).astype(np.int32)
    ok = cls >= 0
    summary = np.array([(length > 0).sum(), (ok & ((cls & 7) == 0)).sum(), (ok & np.isin(cls & 7, (1, 2))).sum(),
                        (ok & ((cls & 7) == 3)).sum(), (cls >= 8).sum(), malformed, over.sum(), 0], np.int32)
    state_out = np.array([int(c["state"][0]) + n, int(c["state"][1]) + c["advance"]], np.int64).astype(np.int32)
    return dict(dg_off=dg_off, dg_len=length, dg_class=cls, summary=summary, state_out=state_out,
                errors=malformed + int(over.sum()))


def tx_rule(c):
    """Every output of the call, datagram by datagram; `data` holds the written datagrams back to back."""
    n = len(c["sched"])
    each = [one_datagram(c, i) for i in range(n)]
    res = place(c, np.array([e[0] for e in each], np.int64).reshape(n), np.array([len(e[1]) for e in each], np.int64).reshape(n))
    res["data"] = np.frombuffer(b"".join(e[1] for e, ln in zip(each, res["dg_len"]) if ln), np.uint8)
    return res


def tx_rule_np(c):
    """tx_rule without a loop over the datagrams."""
    n = len(c["sched"])
    e = c["sched"].astype(np.int64)
    idx = np.arange(n, dtype=np.int64)
    seq = (int(c["state"][0]) + idx) & 0xffff
    pq = np.full(n, -1, np.int64)
    at = c["pong_at"].astype(np.int64)
    inside = (at >= 0) & (at < n)
    pq[at[inside][::-1]] = np.flatnonzero(inside)[::-1]  # (ascending and distinct: one entry each)
    pong = pq >= 0
    hole = e == -1
    okg = (e >= 0) & ((e >> 9) < c["groups"])
    g = np.where(okg, e >> 9, 0)
    x = e & 511
    first = c["first"].astype(np.int64)
    f0, f1 = (first[g], first[g + 1]) if c["groups"] else (np.zeros(n, np.int64), np.zeros(n, np.int64))
    k = f1 - f0
    okk = okg & (f0 >= 0) & (f1 <= c["total"]) & (k >= 1) & (k <= 255)
    is_o, is_r = okk & (x < 256) & (x < k), okk & (x >= 256)
    y = x - 256
    j = np.where(is_o, f0 + x, f0)
    j = np.where(is_o | is_r, j, 0)
    if c["total"]:
        o, ln = c["off"][j], c["ln"][j].astype(np.int64)
    else:
        o, ln = np.zeros(n, np.int64), np.full(n, -1, np.int64)
    pay_ok = (ln >= 0) & (ln <= 65535) & (o >= 0) & (o + ln <= c["payload_bytes"])
    if c["group"] is not None:
        gd = c["group"][g] if c["groups"] else np.zeros(n, DESC)
        ro, mg, Bg = gd["rec_off"].astype(np.int64), gd["m"].astype(np.int64), gd["block_bytes"].astype(np.int64)
    else:
        ro, mg, Bg = g * c["m"] * c["B"], np.full(n, c["m"], np.int64), np.full(n, c["B"], np.int64)
    rm = is_r & ~pong & (mg >= 1) & (y < mg) & (k + mg <= 256)
    k1 = rm & (k == 1) & pay_ok
    rn = (rm & (k >= 2) & (Bg >= 8) & (Bg % 8 == 0) & (Bg <= MAX_BLOCK) & (ro >= 0) & (ro % 8 == 0) &
          (ro + mg * Bg <= c["recovery_bytes"]))
    og = is_o & pay_ok
    cls = np.full(n, -1, np.int64)
    cls[og], cls[rn], cls[k1], cls[hole] = 0, 1, 2, 3
    cls[(og | hole) & pong] += 8
    g7 = (int(c["state"][1]) + g) & 0x7f
    H = np.zeros((n, 14), np.uint8)
    H[:, 0], H[:, 1] = seq & 255, seq >> 8
    wp = (og | hole) & pong
    if wp.any():
        vals = c["pong_val"].reshape(-1, 2)[pq[wp]].astype("<u4")
        H[wp, 2] = 0x81
        H[wp, 3:7] = vals[:, 0:1].copy().view(np.uint8)
        H[wp, 7:11] = vals[:, 1:2].copy().view(np.uint8)
    a0 = np.where(wp, 11, 2)
    rows = np.flatnonzero(og)
    H[rows, a0[rows]], H[rows, a0[rows] + 1], H[rows, a0[rows] + 2] = g7[rows], x[rows], x[rows]
    H[rn, 2], H[rn, 3], H[rn, 4], H[rn, 5] = g7[rn], (k + y)[rn], (k - 1)[rn], (mg - 1)[rn]
    H[k1, 2], H[k1, 3], H[k1, 4] = g7[k1], 1, 0
    hlen = np.zeros(n, np.int64)
    hlen[og], hlen[rn], hlen[k1], hlen[hole & pong] = a0[og] + 3, 6, 5, 11
    blen = np.where(og | k1, ln, np.where(rn, Bg, 0))
    src = np.where(rn, ro + y * Bg, o)
    res = place(c, cls, hlen + blen)
    length = res["dg_len"].astype(np.int64)
    starts = np.cumsum(length) - length
    d = np.repeat(idx, length)
    pos = np.arange(int(length.sum()), dtype=np.int64) - np.repeat(starts, length)
    in_h = pos < hlen[d]
    data = np.zeros(len(d), np.uint8)
    data[in_h] = H[d[in_h], pos[in_h]]
    body = ~in_h
    at = src[d[body]] + pos[body] - hlen[d[body]]
    from_rec = rn[d[body]]
    vals = np.zeros(len(at), np.uint8)
    vals[~from_rec] = c["payload"][at[~from_rec]]
    if from_rec.any():
        vals[from_rec] = c["recovery"][at[from_rec]]
    data[body] = vals
    res["data"] = data
    return res


def ring_image(res, ring_bytes):
    """The ring after the call when every byte of it held CANARY before."""
    ring = np.full(ring_bytes, CANARY, np.uint8)
    length = res["dg_len"].astype(np.int64)
    starts = np.cumsum(length) - length
    pos = np.arange(int(length.sum()), dtype=np.int64) - np.repeat(starts, length)
    ring[np.repeat(res["dg_off"][:-1], length) + pos] = res["data"]
    return ring


def datagrams_of(res):
    length = res["dg_len"].astype(np.int64)
    ends = np.cumsum(length)
    return [res["data"][e - n:e].tobytes() for e, n in zip(ends, length)]


# ---------------------------------------------------------------- traffic for the tests

def pack_payloads(rng, lens, gap=3, lead=1):
    """Payloads of the given lengths in one buffer with random gaps: (buffer, off, payloads)."""
    off, at = [], lead
    for n in lens:
        off.append(at)
        at += n + int(rng.integers(0, gap + 1))
    buf = rng.integers(0, 256, size=at + 1, dtype=np.uint8)
    return buf, np.array(off, np.int64), [buf[o:o + n].tobytes() for o, n in zip(off, lens)]


def interleave(rng, groups_k, groups_m, holes=0):
    """Send order: group g's originals in order, group g - 1's recovery datagrams at random places among
    them, the last group's recovery at the end; `holes` holes at random places."""
    sched = []
    for g, k in enumerate(groups_k + [0]):
        a = [orig(g, x) for x in range(k)]
        b = [recov(g - 1, y) for y in range(groups_m[g - 1])] if g else []
        take = sorted(rng.permutation(len(a) + len(b))[:len(b)].tolist())
        merged, ia, ib = [], iter(a), iter(b)
        for t in range(len(a) + len(b)):
            merged.append(next(ib) if t in take else next(ia))
        sched += merged
    for _ in range(holes):
        sched.insert(int(rng.integers(0, len(sched) + 1)), HOLE)
    return sched


def mixed_case(rng, B, mode, align):
    """Originals, recovery, a k = 1 group, holes, a pong on an original and one on a hole. mode: "uniform",
    "desc" (two different (m, B) in one call) or "norec" (m = 0, no recovery buffer)."""
    ks = [5, 1, 9, 3]
    special = [0, 1, 2, 3, 10, 11, 12, 27, B - 2]
    lens = [v for v in special if 0 <= v <= 65535] + [int(v) for v in rng.integers(0, max(B - 1, 1), size=sum(ks) - len(special))]
    lens = [int(v) for v in rng.permutation(lens[:sum(ks)])]
    payload, off, _ = pack_payloads(rng, lens)
    first = np.concatenate([[0], np.cumsum(ks)])
    if mode == "norec":
        ms = [0] * len(ks)
        kw = dict(m=0, B=B)
    elif mode == "uniform":
        ms = [3] * len(ks)
        kw = dict(m=3, B=B, recovery=rng.integers(0, 256, size=len(ks) * 3 * B, dtype=np.uint8))
    else:
        B2 = B + 8
        ms = [3, 2, 4, 2]
        Bs = [B, B2, B2, B]
        desc, at = [], 8
        for m, b in zip(ms, Bs):
            desc.append((at, m, b))
            at += m * b + 16
        kw = dict(m=0, B=0, group=np.array(desc, DESC), recovery=rng.integers(0, 256, size=at, dtype=np.uint8))
    sched = interleave(rng, ks, ms, holes=3)
    holes = [i for i, e in enumerate(sched) if e == HOLE]
    origs = [i for i, e in enumerate(sched) if e >= 0 and (e & 511) < 256]
    pong_at = sorted([holes[1], origs[2], origs[-1]])
    pong_val = rng.integers(0, 2 ** 32, size=(3, 2), dtype=np.uint64).astype(np.uint32)
    return case(sched, first, payload, off, lens, pong_at=pong_at, pong_val=pong_val,
                state=(int(rng.integers(0, 70000)), int(rng.integers(0, 300))), advance=len(ks), align=align, **kw)


def small_cases():
    rng = np.random.default_rng(5)
    out = []
    for B in (8, 24, 136):
        for mode, align in (("uniform", 1), ("desc", 8), ("norec", 64)):
            out.append(mixed_case(rng, B, mode, align))
    out.append(malformed_case()[0])
    return out


def malformed_case():
    """Every malformed kind of the header once, each between valid neighbours: (case, indices of the bad
    entries)."""
    rng = np.random.default_rng(9)
    ks = [4, 1, 3, 2, 2, 2, 2, 2, 2, 2, 2, 1, 0, 256]  # slot 12: k = 0, slot 13: k = 256
    G = len(ks)
    lens = [int(v) for v in rng.integers(1, 30, size=sum(ks))]
    payload, off, _ = pack_payloads(rng, lens)
    first = np.concatenate([[0], np.cumsum(ks)]).astype(np.int64)
    ln = np.array(lens, np.int64)
    # slot 2: a length past 65535, a span past the buffer's end, a negative offset; slot 11 (k = 1): a bad length
    ln[first[2]] = 65536
    off[first[2] + 1] = len(payload) - int(ln[first[2] + 1]) + 1
    off[first[2] + 2] = -1
    ln[first[11]] = -1
    B = 16
    desc = np.zeros(G, DESC)
    for g in range(G):
        desc[g] = (2 * B * g, 2, B)
    rec_bytes = 2 * B * G
    desc[3]["m"] = 0                 # m_g < 1
    desc[4]["m"] = 255               # k_g + m_g > 256 with k = 2
    desc[5]["block_bytes"] = 4       # B_g < 8
    desc[6]["block_bytes"] = 12      # B_g % 8
    desc[7]["block_bytes"] = MAX_BLOCK + 8
    desc[8]["rec_off"] = -8
    desc[9]["rec_off"] = 12          # not a multiple of 8
    desc[10]["rec_off"] = rec_bytes - 2 * B + 8  # rec_off + m * B > recovery_bytes
    bad = [-2, -2 ** 31, orig(G, 0), 2 ** 31 - 1, orig(0, 4), orig(2, 0), orig(2, 1), orig(2, 2), recov(0, 2), recov(3, 0),
           recov(4, 0), recov(5, 0), recov(6, 0), recov(7, 0), recov(8, 0), recov(9, 0), recov(10, 0), recov(0, 1),
           recov(11, 0), orig(12, 0), recov(12, 0), orig(13, 0), recov(13, 0)]
    good = [orig(0, 0), recov(0, 0), orig(1, 0), recov(1, 1), HOLE, orig(0, 3)]
    sched, where = [], []
    for t, e in enumerate(bad):
        sched.append(good[t % len(good)])
        where.append(len(sched))
        sched.append(e)
    sched.append(good[0])
    pong_at = [where[bad.index(recov(0, 1))]]  # the pong on a recovery entry makes it malformed
    c = case(sched, first, payload, off, ln, recovery=rng.integers(0, 256, size=rec_bytes, dtype=np.uint8), group=desc,
             pong_at=pong_at, pong_val=[7, 9], state=(65530, 125), advance=3, align=8)
    return c, where


# ---------------------------------------------------------------- CPU

def test_tx_symbols_header_and_bindings():
    import shorthair_amd as sh
    for name in ("shorthair_tx_datagram_batch", "shorthair_tx_datagram_scratch_bytes", "shorthair_tx_datagram_capacity"):
        assert name in sh.EXPORTED_SYMBOLS and hasattr(sh.lib, name)
    text = open(os.path.join(INCLUDE, "shorthair_tx.h")).read()
    for name, value in (("SHORTHAIR_TX_TILE", TILE), ("SHORTHAIR_TX_TILE_PASS", TILE_PASS),
                        ("SHORTHAIR_TX_MAX_BLOCK_BYTES", MAX_BLOCK), ("SHORTHAIR_TX_MAX_DATAGRAM_BYTES", MAX_DATAGRAM)):
        assert "#define %s %d " % (name, value) in " ".join(text.split()) + " ", name
    assert (sh.TX_TILE, sh.TX_TILE_PASS, sh.TX_MAX_BLOCK_BYTES, sh.TX_MAX_DATAGRAM_BYTES) == (TILE, TILE_PASS, MAX_BLOCK, MAX_DATAGRAM)
    import ctypes
    assert ctypes.sizeof(sh.TxGroupDesc) == DESC.itemsize == 16


def test_tx_rejects_bad_arguments_without_gpu(capfd):
    """Every host-checked argument: -1, and the GPU is not initialised (nothing on stderr)."""
    import shorthair_amd as sh
    A = 0x7f0000001000  # never dereferenced

    def call(datagrams=40, groups=4, m=2, B=16, total=20, payload_bytes=400, recovery_bytes=4 * 2 * 16, n_pong=1,
             advance=1, align=16, ring_bytes=4096, **ptrs):
        p = dict(sched=A, first=A, payload=A + 1, off=A, len=A, recovery=A, group=A, pong_at=A, pong_val=A, state_in=A,
                 state_out=A, ring=A + 3, dg_off=A, dg_len=A, dg_class=A, summary=A, scratch=A)
        p.update(ptrs)
        return sh.lib.shorthair_tx_datagram_batch(datagrams, groups, m, B, p["sched"], p["first"], total, p["payload"],
                                                  payload_bytes, p["off"], p["len"], p["recovery"], recovery_bytes,
                                                  p["group"], n_pong, p["pong_at"], p["pong_val"], advance, p["state_in"],
                                                  p["state_out"], align, p["ring"], ring_bytes, p["dg_off"], p["dg_len"],
                                                  p["dg_class"], p["summary"], p["scratch"], None)

    for kw in (dict(datagrams=-1), dict(groups=-1), dict(groups=2 ** 22 + 1), dict(m=-1), dict(B=-8), dict(total=-1),
               dict(payload_bytes=-1), dict(recovery_bytes=-1), dict(n_pong=-1), dict(advance=-1), dict(ring_bytes=-1),
               dict(align=0), dict(align=3), dict(align=24), dict(align=8192), dict(align=-16)):
        assert call(**kw) == -1, kw
    for name in ("sched", "first", "len", "pong_at", "pong_val", "state_in", "state_out", "dg_len", "dg_class", "summary"):
        assert call(**{name: A + 2}) == -1, name
    for name in ("off", "group", "recovery", "dg_off", "scratch"):
        assert call(**{name: A + 4}) == -1, name
    for name in ("state_in", "state_out", "dg_off", "summary", "scratch", "sched", "dg_len", "dg_class", "first", "off",
                 "len", "payload", "recovery", "ring", "pong_at", "pong_val"):
        assert call(**{name: None}) == -1, name
    assert call(datagrams=0, sched=None, state_in=None) == -1  # the state is written even for an empty batch
    assert sh.lib.shorthair_tx_datagram_scratch_bytes(-1) == -1
    for args in ((-1, 10, 1), (1, -1, 1), (1, 10, 0), (1, 10, 3), (1, 10, 8192)):
        assert sh.lib.shorthair_tx_datagram_capacity(*args) == -1, args
    with pytest.raises(ValueError):
        sh.tx_datagram_scratch_bytes(-1)
    with pytest.raises(ValueError):
        sh.tx_datagram_capacity(1, 1, 5)
    assert capfd.readouterr().err == ""


def test_tx_scratch_and_capacity_queries():
    import shorthair_amd as sh
    ns = [0, 1, TILE - 1, TILE, TILE + 1, TILE * TILE_PASS, TILE * TILE_PASS + 1, 2 ** 20 + 100, 2 ** 31 - 1]
    sizes = [sh.tx_datagram_scratch_bytes(n) for n in ns]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and all(s % 8 == 0 for s in sizes)
    for align in (1, 2, 16, 64, 4096):
        prev = -1
        for n in ns:
            for mx in (0, 1, 11, 1403, MAX_DATAGRAM):
                cap = sh.tx_datagram_capacity(n, mx, align)
                assert cap == n * roundup(mx, align)
            assert sh.tx_datagram_capacity(n, 1403, align) >= prev
            prev = sh.tx_datagram_capacity(n, 1403, align)
    # the rule's worst case: the longest original with a pong, and the largest recovery block, at every alignment
    assert 14 + 65535 <= MAX_DATAGRAM and 6 + MAX_BLOCK <= MAX_DATAGRAM
    rng = np.random.default_rng(2)
    for align in (1, 16, 4096):
        lens = [65535, 65535]
        payload, off, _ = pack_payloads(rng, lens)
        c = case([orig(0, 0), orig(0, 1), recov(0, 0), recov(0, 1)], [0, 2], payload, off, lens, m=2, B=MAX_BLOCK,
                 recovery=np.zeros(2 * MAX_BLOCK, np.uint8), pong_at=[0, 1], pong_val=[1, 2, 3, 4], align=align)
        res = tx_rule_np(c)
        assert res["dg_len"].tolist() == [14 + 65535] * 2 + [6 + MAX_BLOCK] * 2
        assert res["dg_off"][-1] <= sh.tx_datagram_capacity(4, MAX_DATAGRAM, align)


def test_tx_numpy_form_equals_the_sequential_rule():
    for t, c in enumerate(small_cases()):
        for ring_bytes in (None, 200, 0):
            c = dict(c, ring_bytes=ring_bytes)
            a, b = tx_rule(c), tx_rule_np(c)
            for name in a:
                assert np.array_equal(a[name], b[name]), (t, ring_bytes, name)
    c, where = malformed_case()
    res = tx_rule(c)
    assert (res["dg_class"][where] == -1).all() and (res["dg_len"][where] == 0).all()
    assert (np.delete(res["dg_class"], where) >= 0).all() and res["summary"][5] == len(where)


@functools.lru_cache(maxsize=None)
def fixture():
    """tests/golden/tx_datagrams.npz parsed into a schedule: (case without recovery, per slot (k, m, B, payloads),
    the reference's datagrams, which of them are holes)."""
    z = np.load(FIXTURE)

    def split(name):
        ends = np.cumsum(z[name + "_len"].astype(np.int64))
        return [z[name + "_bytes"][e - n:e].tobytes() for e, n in zip(ends, z[name + "_len"])]

    dgs, pays, oobs = split("dg"), split("pay"), split("oob")
    sched, pong_at, pong_val, hole = [], [], [], []
    u = 0
    slots = {}  # unwrapped group -> dict(ids, m, B, k1)
    for i, d in enumerate(dgs):
        assert d[0] | (d[1] << 8) == i & 0xffff
        rest = d[2:]
        has_pong = bool(rest[0] & 0x80 and rest[0] & 1)
        if has_pong:
            vals = (int.from_bytes(rest[1:5], "little"), int.from_bytes(rest[5:9], "little"))
            rest = rest[9:]
        if not rest or rest[0] & 0x80:  # pong only, or out of band: the host's datagram
            if has_pong and not rest:
                pong_at.append(i)
                pong_val.append(vals)
            sched.append(HOLE)
            hole.append(bool(rest))
            continue
        hole.append(False)
        u = expand(u, rest[0])
        s = slots.setdefault(u, dict(ids=[], m=0, B=0, k1=0, k=None))
        rid, c_ = rest[1], rest[2]
        if rid <= c_:
            assert rid == c_ == len(s["ids"])
            s["ids"].append(rid)
            sched.append(orig(u, rid))
            if has_pong:
                pong_at.append(i)
                pong_val.append(vals)
        else:
            assert not has_pong
            k = c_ + 1
            assert k == len(s["ids"])
            if k == 1:
                sched.append(recov(u, s["k1"]))
                s["k1"] += 1
                s["m"] = s["k1"]
            else:
                s["m"], s["B"] = rest[3] + 1, len(rest) - 4
                sched.append(recov(u, rid - k))
    G = max(slots) + 1
    ks = [len(slots[g]["ids"]) if g in slots else 0 for g in range(G)]
    assert sum(ks) == len(pays) and sum(hole) == len(oobs)
    first = np.concatenate([[0], np.cumsum(ks)])
    lens = [len(p) for p in pays]
    payload = np.frombuffer(b"".join(pays), np.uint8)
    off = np.cumsum([0] + lens[:-1])
    per_slot = [(ks[g], slots[g]["m"] if g in slots else 0, slots[g]["B"] if g in slots else 0,
                 pays[first[g]:first[g + 1]]) for g in range(G)]
    c = case(sched, first, payload, off, lens, pong_at=pong_at, pong_val=pong_val, state=(0, 0), advance=G)
    return c, per_slot, dgs, hole


def with_recovery(c, per_slot, blocks_of):
    """The case with one recovery buffer described per slot; blocks_of(g, k, m, B, payloads) -> m blocks."""
    desc, parts, at = np.zeros(len(per_slot), DESC), [], 0
    for g, (k, m, B, pays) in enumerate(per_slot):
        desc[g] = (at, m, B)
        if k >= 2 and m:
            blocks = blocks_of(g, k, m, B, pays)
            assert len(blocks) == m and all(len(b) == B for b in blocks)
            parts += blocks
            at += m * B
    rec = np.frombuffer(b"".join(parts), np.uint8)
    return dict(c, group=desc, recovery=rec, recovery_bytes=len(rec))


def test_fixture_rule_reproduces_the_reference_datagrams():
    """tx_rule on the schedule parsed from the reference's own traffic, with recovery blocks from the packet
    oracle: every datagram that is not a hole is the reference's, byte for byte."""
    c, per_slot, dgs, hole = fixture()
    ora = po.oracle()
    assert len(c["pong_at"]) >= 2 and len({(m, B) for k, m, B, _ in per_slot if k >= 2 and m}) >= 2

    def blocks_of(g, k, m, B, pays):
        return [p[3:] for p in opk.tx_group(ora, m, pays)]

    res = tx_rule(with_recovery(c, per_slot, blocks_of))
    assert res["summary"][5] == 0 and res["summary"][6] == 0
    got = datagrams_of(res)
    n_compared = 0
    for i, (d, h) in enumerate(zip(dgs, hole)):
        if h:
            assert got[i] == b"" and res["dg_class"][i] == 3
        else:
            assert got[i] == d, i
            n_compared += 1
    assert n_compared == len(dgs) - sum(hole) > 2000 and (res["dg_class"] >= 8).sum() >= 2


# ---------------------------------------------------------------- running on the GPU

@pytest.fixture(scope="module")
def sh():
    import torch
    import shorthair_amd
    assert shorthair_amd.cauchy_256_init() == 0
    torch.cuda.init()
    return shorthair_amd


OUTS = ("dg_off", "dg_len", "dg_class", "summary", "state_out")


def run_tx(sh, c, ring_mis=0, variant=0, payload_mis=1, ring_bytes=None, alias=False):
    """Runs the call with every array between canaries (variant 0: bases of the least alignment the contract
    allows; 1: 16-byte aligned), the ring at ring_mis (mod 16) and filled with CANARY; checks the canaries and
    that the inputs are unchanged. Returns (rc, outputs incl. `ring` and `errors`)."""
    import torch
    lo = variant == 0
    i4, i8 = (4, 8) if lo else (0, 0)
    n = len(c["sched"])
    if ring_bytes is None:
        ring_bytes = int(tx_rule_np(dict(c, ring_bytes=None))["dg_off"][-1]) if c["ring_bytes"] is None else c["ring_bytes"]
    G = c["groups"]
    ins = dict(sched=Guarded(4 * n, i4, c["sched"]), first=Guarded(4 * len(c["first"]), i4 + 8 * lo, c["first"]),
               payload=Guarded(len(c["payload"]), payload_mis, c["payload"]), off=Guarded(8 * len(c["off"]), i8, c["off"]),
               ln=Guarded(4 * len(c["ln"]), i4, c["ln"]),
               pong_at=Guarded(4 * len(c["pong_at"]), i4, c["pong_at"]),
               pong_val=Guarded(4 * len(c["pong_val"]), i4 + 8 * lo, c["pong_val"]))
    if c["recovery"] is not None:
        ins["recovery"] = Guarded(len(c["recovery"]), i8, c["recovery"])
    if c["group"] is not None:
        ins["group"] = Guarded(16 * len(c["group"]), i8, c["group"])
    state = Guarded(8, i4, c["state"])
    outs = dict(dg_off=(Guarded(8 * (n + 1), i8), np.int64), dg_len=(Guarded(4 * n, i4), np.int32),
                dg_class=(Guarded(4 * n, i4 + 8 * lo), np.int32), summary=(Guarded(32, i4), np.int32),
                state_out=(state if alias else Guarded(8, i4 + 8 * lo), np.int32), ring=(Guarded(ring_bytes, ring_mis), np.uint8))
    scratch = Guarded(sh.tx_datagram_scratch_bytes(n), i8)
    P = lambda name: ins[name].ptr if name in ins and ins[name].n else None  # noqa: E731
    sh.batch_errors()
    rc = sh.lib.shorthair_tx_datagram_batch(
        n, G, c["m"], c["B"], P("sched"), ins["first"].ptr if len(c["first"]) else None, c["total"],
        ins["payload"].ptr if c["payload_bytes"] else None, c["payload_bytes"], P("off"), P("ln"), P("recovery"),
        c["recovery_bytes"], P("group"), len(c["pong_at"]), P("pong_at"), P("pong_val"), c["advance"], state.ptr,
        outs["state_out"][0].ptr, c["align"], outs["ring"][0].ptr if ring_bytes else None, ring_bytes,
        outs["dg_off"][0].ptr, outs["dg_len"][0].ptr if n else None, outs["dg_class"][0].ptr if n else None,
        outs["summary"][0].ptr, scratch.ptr, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    scratch.read(np.uint8)  # canaries
    for name, gd in ins.items():
        assert gd.unchanged(), name
    if not alias:
        assert state.unchanged()
    got = {name: gd.read(dt) for name, (gd, dt) in outs.items()}
    got["errors"] = sh.batch_errors()
    return rc, got


def check(sh, c, tag, rule=tx_rule, **kw):
    """The call against the rule: every output element, the ring gap bytes included."""
    rc, got = run_tx(sh, c, **kw)
    assert rc == 0, tag
    want = rule(dict(c, ring_bytes=len(got["ring"])))
    for name in OUTS:
        assert got[name].shape == want[name].shape, (tag, name)
        bad = np.flatnonzero(got[name] != want[name])
        assert not len(bad), (tag, name, bad[:6], got[name][bad[:6]], want[name][bad[:6]])
    image = ring_image(want, len(got["ring"]))
    bad = np.flatnonzero(got["ring"] != image)
    assert not len(bad), (tag, "ring", bad[:8], got["ring"][bad[:8]], image[bad[:8]])
    assert got["errors"] == want["errors"], tag
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["uniform", "desc", "norec"])
@pytest.mark.parametrize("B", [8, 16, 24, 136, 1352])
def test_tx_rule_matrix(sh, B, mode):
    """Originals, recovery, a k = 1 group, holes, a pong on an original and on a hole; payload lengths 0, 1, 2,
    3, 10, 11, 12, 27, B - 2 and random ones; the ring at all 16 addresses mod 16, the payload buffer at odd
    addresses, align 1, 8, 16 and 64."""
    rng = np.random.default_rng(B * 7 + len(mode))
    for mis in range(16):
        align = (1, 8, 16, 64)[(mis + mis // 4) % 4]
        c = mixed_case(rng, B, mode, align)
        want = check(sh, c, (B, mode, mis, align), ring_mis=mis, variant=mis & 1, payload_mis=(2 * mis + 1) % 16)
        assert want["summary"][4] == 3 and want["summary"][3] == 3 and want["summary"][5] == 0 and want["errors"] == 0
        if mode == "norec":
            assert c["recovery"] is None and not np.isin(want["dg_class"], (1, 2)).any()
        else:
            assert (want["dg_class"] == 1).any() and (want["dg_class"] == 2).any()


@pytest.mark.gpu
def test_tx_every_malformed_kind(sh):
    """Each malformed kind once between valid neighbours: class -1, length 0, counted, nothing written."""
    c, where = malformed_case()
    for variant in (0, 1):
        want = check(sh, c, ("malformed", variant), ring_mis=5 * variant, variant=variant)
        assert (want["dg_class"][where] == -1).all() and want["summary"][5] == len(where) == want["errors"]
        assert (np.delete(want["dg_class"], where) >= 0).all()
    # a span outside [0, total_blocks]: the same arrays with total_blocks cut to slot 0's span, so that the
    # valid entries of slot 1 become malformed too
    cut = dict(c, total=int(c["first"][1]))
    want = check(sh, cut, "span")
    named = np.array([e >= 0 and (e >> 9) >= 1 for e in c["sched"]])
    assert (want["dg_class"][named] == -1).all() and want["summary"][5] > len(where)


@pytest.mark.gpu
def test_tx_ring_too_small(sh):
    """The ring ends inside a datagram: that one and every later one of non-zero length is class -2 with
    length 0 and is not written -- the offsets ascend and keep the rule's lengths, so no later datagram of
    non-zero length can fit --, a hole behind them stays a hole, and d_dg_off[n] is still the need."""
    rng = np.random.default_rng(31)
    c = mixed_case(rng, 136, "uniform", 16)
    c["sched"] = np.concatenate([c["sched"], [HOLE, orig(0, 1)]]).astype(np.int32)
    full = tx_rule(c)
    need = int(full["dg_off"][-1])
    for cut_at in (len(c["sched"]) // 2, 1):
        for inside in (1, -1):  # the ring ends one byte short of datagram cut_at, or one byte into it
            lim = int(full["dg_off"][cut_at]) + (int(full["dg_len"][cut_at]) - 1 if inside > 0 else 1)
            want = check(sh, dict(c, ring_bytes=lim), ("small", cut_at, inside), ring_mis=3)
            assert want["dg_off"][-1] == need and want["summary"][6] > 0
            assert (want["dg_class"][cut_at:][full["dg_len"][cut_at:] > 0] == -2).all()
            assert (want["dg_class"][:cut_at] == full["dg_class"][:cut_at]).all() and want["dg_class"][-2] == 3
    want = check(sh, dict(c, ring_bytes=0), "no ring")
    assert want["summary"][0] == 0


def tiny_case(rng, n, state=(0, 0), align=1, groups=3, holes=True):
    """n datagrams of a few bytes: originals of 0..3 bytes, k = 1 forms, holes, some with a pong."""
    ks = [1] + [4] * (groups - 1)
    lens = [int(v) for v in rng.integers(0, 4, size=sum(ks))]
    payload, off, _ = pack_payloads(rng, lens)
    first = np.concatenate([[0], np.cumsum(ks)])
    pool = np.array([orig(g, x) for g in range(groups) for x in range(ks[g])] + [recov(0, 0), recov(0, 1)] + [HOLE] * holes, np.int32)
    sched = pool[rng.integers(0, len(pool), size=n)]
    pong_at = np.flatnonzero((rng.integers(0, 50, size=n) == 0) & ((sched & 511) < 256))
    return case(sched, first, payload, off, lens, m=2, B=8, pong_at=pong_at,
                pong_val=rng.integers(0, 2 ** 32, size=2 * len(pong_at), dtype=np.uint64).astype(np.uint32),
                state=state, advance=groups, align=align)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, TILE - 1, TILE, TILE + 1])
def test_tx_datagram_counts(sh, n):
    rng = np.random.default_rng(n)
    c = tiny_case(rng, n, state=(65535 - n // 2, 127 - 1))  # the sequence number wraps inside the batch
    want = check(sh, c, n, ring_mis=7, alias=bool(n & 1))
    assert want["state_out"].tolist() == [65535 - n // 2 + n, 126 + 3] and want["dg_off"].shape == (n + 1,)


@pytest.mark.gpu
def test_tx_tile_pass_boundary(sh):
    """TILE_PASS * TILE + 1 tiny datagrams: the scan workgroup takes a second pass for one tile of one datagram."""
    rng = np.random.default_rng(77)
    c = tiny_case(rng, TILE_PASS * TILE + 1, state=(1000, 5), align=8)
    want = check(sh, c, "pass", rule=tx_rule_np, ring_mis=9)
    assert want["summary"][0] > 200000 and want["summary"][4] > 1000


@pytest.mark.gpu
def test_tx_sequence_and_group_byte_wrap(sh):
    """seq 65535 -> 0 and the group byte 127 -> 0 inside one batch."""
    rng = np.random.default_rng(3)
    ks = [3, 3, 3, 3]
    lens = [int(v) for v in rng.integers(5, 20, size=12)]
    payload, off, _ = pack_payloads(rng, lens)
    sched = interleave(rng, ks, [2] * 4)
    c = case(sched, np.concatenate([[0], np.cumsum(ks)]), payload, off, lens, m=2, B=24,
             recovery=rng.integers(0, 256, size=4 * 2 * 24, dtype=np.uint8), state=(65535 - 7, 126), advance=4, align=16)
    want = check(sh, c, "wrap", ring_mis=2)
    dgs = datagrams_of(want)
    seqs = [d[0] | (d[1] << 8) for d in dgs]
    assert seqs == [(65528 + i) & 0xffff for i in range(len(dgs))] and 0 in seqs and 65535 in seqs
    assert {d[2] for d in dgs} == {126, 127, 0, 1} and want["state_out"].tolist() == [65528 + len(dgs), 130]


@pytest.mark.gpu
def test_tx_largest_block(sh):
    """B = 65,544 and a payload of 65,535 bytes with a pong: the longest datagrams there are."""
    rng = np.random.default_rng(4)
    lens = [65535, 17]
    payload, off, _ = pack_payloads(rng, lens)
    c = case([orig(0, 0), recov(0, 1), orig(0, 1), recov(0, 0)], [0, 2], payload, off, lens, m=2, B=MAX_BLOCK,
             recovery=rng.integers(0, 256, size=2 * MAX_BLOCK, dtype=np.uint8), pong_at=[0], pong_val=[5, 6], align=64)
    want = check(sh, c, "largest", rule=tx_rule_np, ring_mis=11)
    assert want["dg_len"].tolist() == [14 + 65535, 6 + MAX_BLOCK, 5 + 17, 6 + MAX_BLOCK]


@pytest.mark.gpu
def test_tx_offsets_past_4_gib(sh):
    """align = 4096 with 2^20 + 100 short datagrams: the ring is above 4 GiB and the last offsets need more than
    32 bits. The ring is allocated uninitialised and only the datagrams' own bytes are gathered on the device
    and compared: no canary is possible in a ring of this size, so stray writes into gaps are not seen here
    (the small cases check them)."""
    import torch
    n = 2 ** 20 + 100
    rng = np.random.default_rng(8)
    c = tiny_case(rng, n, state=(40000, 100), align=4096, groups=5, holes=False)
    want = tx_rule_np(c)
    ring_bytes = int(want["dg_off"][-1])
    assert ring_bytes > 2 ** 32 and want["dg_off"][-2] > 2 ** 32 and want["dg_len"].max() <= 32
    ring = torch.empty(ring_bytes, dtype=torch.uint8, device="cuda")
    t = dv(c, ("sched", "first", "payload", "off", "ln", "pong_at", "pong_val", "state"))
    dg_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    dg_len, dg_class = (torch.full((n,), -9, dtype=torch.int32, device="cuda") for _ in range(2))
    summary, state_out = (torch.full((k,), -9, dtype=torch.int32, device="cuda") for k in (8, 2))
    scratch = torch.empty(sh.tx_datagram_scratch_bytes(n), dtype=torch.uint8, device="cuda")
    sh.batch_errors()
    assert sh.tx_datagram_batch(n, c["groups"], c["m"], c["B"], t["sched"], t["first"], c["total"], t["payload"],
                                c["payload_bytes"], t["off"], t["ln"], None, 0, None, len(c["pong_at"]), t["pong_at"],
                                t["pong_val"], c["advance"], t["state"], state_out, 4096, ring, ring_bytes, dg_off, dg_len,
                                dg_class, summary, scratch) == 0
    got = dict(dg_off=dg_off, dg_len=dg_len, dg_class=dg_class, summary=summary, state_out=state_out)
    for name in OUTS:
        assert np.array_equal(got[name].cpu().numpy(), want[name]), name
    # datagrams 0 .. n - 2 start at multiples of 4096 (no datagram is longer), the last wherever
    assert (want["dg_off"][:-1] == 4096 * np.cumsum(np.concatenate([[0], want["dg_len"][:-1] > 0]))).all()
    rows = int((want["dg_len"] > 0).sum())
    heads = ring[:rows * 4096].view(rows, 4096)[:, :32].contiguous().cpu().numpy()
    length = want["dg_len"][want["dg_len"] > 0].astype(np.int64)
    mask = np.arange(32)[None, :] < length[:, None]
    assert np.array_equal(heads[mask], want["data"])
    assert sh.batch_errors() == want["errors"]


# ---------------------------------------------------------------- GPU: the reference's bytes

def dv(c, names):
    """The case's arrays on the device (uint32 as its int32 view)."""
    return {k: _dev(c[k].view(np.int32) if c[k].dtype == np.uint32 else c[k]) for k in names}


def dev_frame_encode(sh, kmax, m, B, first, payload, off, ln):
    """frame -> var-k encode on the device: the recovery blocks [groups][m][B] as a tensor."""
    import torch
    G, total = len(first) - 1, int(first[-1])
    blocks = torch.zeros((total, B), dtype=torch.uint8, device="cuda")
    assert sh.frame_batch(B, total, payload, payload.numel(), _dev(np.asarray(off, np.int64)), _dev(np.asarray(ln, np.int32)),
                          None, blocks) == 0
    rec = torch.zeros((G, m, B), dtype=torch.uint8, device="cuda")
    assert sh.encode_batch_var(kmax, m, B, G, _dev(np.asarray(first, np.int32)), total, blocks, rec) == 0
    return rec


def dev_tx(sh, c, d, ring, state_in, state_out):
    """The call on tensors (d: the case's arrays on the device). Returns dg_off, dg_len, dg_class, summary."""
    import torch
    n = len(c["sched"])
    dg_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    dg_len, dg_class = (torch.full((n,), -9, dtype=torch.int32, device="cuda") for _ in range(2))
    summary = torch.full((8,), -9, dtype=torch.int32, device="cuda")
    scratch = torch.full((sh.tx_datagram_scratch_bytes(n),), 0x77, dtype=torch.uint8, device="cuda")
    assert sh.tx_datagram_batch(n, c["groups"], c["m"], c["B"], d["sched"], d["first"], c["total"], d["payload"],
                                c["payload_bytes"], d["off"], d["ln"], d.get("recovery"), c["recovery_bytes"],
                                d.get("group"), len(c["pong_at"]), d.get("pong_at"), d.get("pong_val"), c["advance"],
                                state_in, state_out, c["align"], ring, ring.numel(), dg_off, dg_len, dg_class, summary,
                                scratch) == 0
    return dg_off, dg_len, dg_class, summary


@pytest.mark.gpu
def test_fixture_datagrams_on_the_device(sh):
    """The fixture's payloads framed with shorthair_frame_batch, one cauchy_256_encode_batch_var per (m, B) bucket
    into one recovery buffer described by d_group, one shorthair_tx_datagram_batch: every datagram that is not
    a hole is the reference's, byte for byte."""
    import torch
    c, per_slot, dgs, hole = fixture()
    payload = _dev(c["payload"])
    buckets = sorted({(m, B) for k, m, B, _ in per_slot if k >= 2 and m})
    desc, parts, at = np.zeros(len(per_slot), DESC), [], 0
    for g, (k, m, B, _) in enumerate(per_slot):
        desc[g] = (0, m, B)
    for m, B in buckets:
        members = [g for g, (k, gm, gB, _) in enumerate(per_slot) if k >= 2 and (gm, gB) == (m, B)]
        idx = np.concatenate([np.arange(c["first"][g], c["first"][g + 1]) for g in members])
        first = np.concatenate([[0], np.cumsum([per_slot[g][0] for g in members])])
        parts.append(dev_frame_encode(sh, max(per_slot[g][0] for g in members), m, B, first, payload, c["off"][idx],
                                      c["ln"][idx]).reshape(-1))
        for t, g in enumerate(members):
            desc[g]["rec_off"] = at + t * m * B
        at += len(members) * m * B
    rec = torch.cat(parts)
    c = dict(c, group=desc, recovery_bytes=rec.numel(), align=16)
    d = dv(c, ("sched", "first", "off", "ln", "pong_at", "pong_val"))
    d.update(payload=payload, recovery=rec, group=_dev(desc.view(np.uint8)))
    ring = torch.full((sh.tx_datagram_capacity(len(dgs), max(len(x) for x in dgs), 16),), CANARY, dtype=torch.uint8, device="cuda")
    state = torch.zeros(2, dtype=torch.int32, device="cuda")
    sh.batch_errors()
    dg_off, dg_len, dg_class, summary = dev_tx(sh, c, d, ring, state, state)
    assert sh.batch_errors() == 0
    ring_h, dg_off, dg_len, dg_class = (x.cpu().numpy() for x in (ring, dg_off, dg_len, dg_class))
    for i, (want, h) in enumerate(zip(dgs, hole)):
        if h:
            assert dg_len[i] == 0 and dg_class[i] == 3
        else:
            assert ring_h[dg_off[i]:dg_off[i] + dg_len[i]].tobytes() == want, i
    assert state.cpu().tolist() == [len(dgs), len(per_slot)] and summary.cpu()[0] == len(dgs) - sum(hole)


# ---------------------------------------------------------------- GPU: the loop on the device

LOOP = [(28, 4, 136, "fixed"), (30, 6, 136, "tile"), (20, 4, 24, "generic")]


def loop_traffic(rng, kmax, m, B, G):
    ks = [int(v) for v in rng.integers(max(2, kmax - 6), kmax + 1, size=G)]
    # (no empty payload: the receiver drops a data datagram of five bytes as short, as OnData does)
    lens = [int(v) for v in rng.integers(1, B - 1, size=sum(ks))]
    lens[0], lens[1] = B - 2, 1
    payload, off, pays = pack_payloads(rng, lens)
    first = np.concatenate([[0], np.cumsum(ks)])
    dropped = [set(rng.permutation(ks[g])[:g % (m + 1)].tolist()) for g in range(G)]  # e_g <= m originals of group g
    return ks, lens, payload, off, pays, first, dropped


def receive(sh, ring, dg_off, dg_len, keep, U0, G, kmax, m, B):
    """drop -> group -> list -> frame -> decode -> unframe on the device: per slot (surviving originals,
    recovered). The drop leaves the (off, len) pairs of the dropped datagrams out, on the device."""
    import torch
    keep = _dev(np.asarray(keep, np.int64))
    k_off, k_len = dg_off[keep].contiguous(), dg_len[keep].contiguous()
    state = _dev(np.array([U0], np.int32))
    grp = dev_group(sh, ring, k_off, k_len, state, torch.zeros(1, dtype=torch.int32, device="cuda"), G, 0)
    _, recovered = dev_bucket(sh, ring, len(keep), G, grp, 2, kmax, m, B)
    records = slot_records(ring.cpu().numpy(), grp, G)
    return [([(r[0], r[2:]) for r in records[s] if r[0] <= r[1]], recovered.get(s)) for s in range(G)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", LOOP, ids=lambda s: "k%d_m%d_B%d_%s" % s)
def test_tx_loop_on_the_device(sh, shape):
    """frame -> encode -> tx datagrams -> drop -> rx group -> list -> frame -> decode -> unframe with nothing but
    scalars from the host: what is delivered is what the packet oracle delivers, and with the surviving
    originals it is every payload sent. Then again with the sender's side cut into two batches, d_state_out fed
    forward and `advance` the number of groups the first batch has finished."""
    import torch
    kmax, m, B, route = shape
    assert sh.path(kmax, m, B) == route
    G, U0 = 7, 125
    rng = np.random.default_rng(kmax + m)
    ora = po.oracle()
    ks, lens, payload_h, off, pays, first, dropped = loop_traffic(rng, kmax, m, B, G)
    sched = interleave(rng, ks, [m] * G, holes=2)
    payload = _dev(payload_h)
    rec = dev_frame_encode(sh, kmax, m, B, first, payload, off, lens)
    c = case(sched, first, payload_h, off, lens, m=m, B=B, recovery_bytes=rec.numel(), state=(65500, U0), advance=G, align=8)
    d = dv(c, ("sched", "first", "off", "ln"))
    d.update(payload=payload, recovery=rec)
    ring = torch.full((sh.tx_datagram_capacity(len(sched), 6 + B, 8),), CANARY, dtype=torch.uint8, device="cuda")
    state = _dev(c["state"])
    sh.batch_errors()
    dg_off, dg_len, dg_class, summary = dev_tx(sh, c, d, ring, state, state)
    assert summary.cpu().tolist() == [len(sched) - 2, sum(ks), G * m, 2, 0, 0, 0, 0]
    assert state.cpu().tolist() == [65500 + len(sched), U0 + G]
    keep = [i for i, e in enumerate(sched) if e >= 0 and not ((e & 511) < 256 and (e & 511) in dropped[e >> 9])]
    # what the packet oracle delivers from the same arrivals
    want = []
    for g in range(G):
        gp = pays[first[g]:first[g + 1]]
        wire = opk.tx_group(ora, m, gp)
        arrived = [e & 511 for i, e in enumerate(sched) if i in set(keep) and e >> 9 == g]
        want.append(([(x, gp[x]) for x in arrived if x < 256], opk.rx_group(ora, [(x, gp[x]) for x in arrived if x < 256],
                                                                           [wire[x - 256] for x in arrived if x >= 256])))
    got = receive(sh, ring, dg_off[:-1], dg_len, keep, U0, G, kmax, m, B)
    for g in range(G):
        assert got[g][0] == want[g][0], g
        assert sorted(got[g][1] or []) == sorted(want[g][1] or []) and (got[g][1] is None) == (want[g][1] is None), g
        everything = dict(got[g][0] + (got[g][1] or []))
        assert everything == dict(enumerate(pays[first[g]:first[g + 1]])), g
    assert any(w[1] for w in want) and want[0][1] is None
    single = [ring.cpu().numpy()[o:o + n].tobytes() for o, n in zip(dg_off.cpu().numpy(), dg_len.cpu().numpy())]
    # two batches: the first ends when slot `a` has sent its originals and slot a - 1 its recovery; slot a is slot 0 of the second batch,
    # which sends its recovery, so the first batch has finished `a` groups
    a = 3
    cut = min(i for i, e in enumerate(sched) if e >= 0 and (e >> 9 == a + 1 or (e >> 9 == a and (e & 511) >= 256)))
    assert all(e < 0 or e >> 9 >= a for e in sched[cut:])
    state.copy_(_dev(c["state"]))
    ring2 = torch.full_like(ring, CANARY)
    c1 = dict(c, sched=np.asarray(sched[:cut], np.int32), groups=a + 1, advance=a)
    d1 = dict(d, sched=_dev(c1["sched"]))
    off1, len1, _, sum1 = dev_tx(sh, c1, d1, ring2, state, state)
    base = int(off1.cpu()[-1])
    c2 = dict(c, sched=np.asarray([e if e < 0 else e - (a << 9) for e in sched[cut:]], np.int32), groups=G - a, advance=G - a,
              recovery_bytes=rec.numel() - a * m * B)
    d2 = dict(d, sched=_dev(c2["sched"]), first=d["first"][a:], recovery=rec.reshape(-1)[a * m * B:])
    off2, len2, _, sum2 = dev_tx(sh, c2, d2, ring2[base:], state, state)
    assert state.cpu().tolist() == [65500 + len(sched), U0 + G] and sh.batch_errors() == 0
    both_off = torch.cat([off1[:-1], off2[:-1] + base])
    both_len = torch.cat([len1, len2])
    r2 = ring2.cpu().numpy()
    assert [r2[o:o + n].tobytes() for o, n in zip(both_off.cpu().numpy(), both_len.cpu().numpy())] == single
    got2 = receive(sh, ring2, both_off, both_len, keep, U0, G, kmax, m, B)
    assert got2 == got


# ---------------------------------------------------------------- GPU: the binding on tensors, in a graph

@pytest.mark.gpu
def test_tx_python_binding_on_tensors_and_graph_replay(sh):
    """One captured call with aliased state, replayed twice with d_sched rewritten in between: the second
    replay's sequence numbers and group bytes continue from the first, and the outputs are the rule's."""
    import torch
    rng = np.random.default_rng(12)
    c = mixed_case(rng, 136, "desc", 16)
    n = len(c["sched"])
    c["advance"] = 5
    s = torch.cuda.Stream()
    d = dv(c, ("sched", "first", "payload", "off", "ln", "recovery", "pong_at", "pong_val"))
    d["group"] = _dev(c["group"].view(np.uint8))
    state = _dev(c["state"])
    ring_bytes = sh.tx_datagram_capacity(n, 14 + 6 + 136 + 8, 16)
    outs = dict(dg_off=(Guarded(8 * (n + 1), 8), torch.int64), dg_len=(Guarded(4 * n, 4), torch.int32),
                dg_class=(Guarded(4 * n, 12), torch.int32), summary=(Guarded(32, 4), torch.int32),
                ring=(Guarded(ring_bytes, 5), torch.uint8))
    t = {name: g.tensor(dt) for name, (g, dt) in outs.items()}
    scratch = Guarded(sh.tx_datagram_scratch_bytes(n), 8)
    torch.cuda.synchronize()

    def run():
        assert sh.tx_datagram_batch(n, c["groups"], 0, 0, d["sched"], d["first"], c["total"], d["payload"], c["payload_bytes"],
                                    d["off"], d["ln"], d["recovery"], c["recovery_bytes"], d["group"], len(c["pong_at"]),
                                    d["pong_at"], d["pong_val"], c["advance"], state, state, 16, t["ring"], ring_bytes,
                                    t["dg_off"], t["dg_len"], t["dg_class"], t["summary"], scratch.tensor(torch.uint8)) == 0

    def check_now(sched_now, state_now, tag):
        want = tx_rule(dict(c, sched=sched_now, state=np.asarray(state_now, np.int32), ring_bytes=ring_bytes))
        got = {name: g.read(np.dtype(str(dt).split(".")[1])) for name, (g, dt) in outs.items()}
        scratch.read(np.uint8)
        for name in ("dg_off", "dg_len", "dg_class", "summary"):
            assert np.array_equal(got[name], want[name]), (tag, name)
        assert np.array_equal(got["ring"], ring_image(want, ring_bytes)), tag
        assert state.cpu().tolist() == want["state_out"].tolist(), tag
        return want

    sh.batch_errors()
    with torch.cuda.stream(s):
        run()  # loads the kernels' code and creates the stream's error counter before the capture
    s.synchronize()
    check_now(c["sched"], c["state"], "eager")
    state_now = [int(c["state"][0]) + n, int(c["state"][1]) + 5]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        run()
    errors = 0
    for rep in range(2):
        sched_now = c["sched"].copy()
        sched_now[rng.permutation(n)[:4]] = [HOLE, -7, orig(0, 1), recov(2, 0)]
        sched_now = np.roll(sched_now, 3 + rep)
        d["sched"].copy_(torch.from_numpy(sched_now))
        for name, v in t.items():
            v.fill_(CANARY if name == "ring" else 5)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        want = check_now(sched_now, state_now, rep)
        assert want["summary"][0] > 10
        errors += want["errors"]
        state_now = [state_now[0] + n, state_now[1] + 5]
    assert sh.batch_errors(s.cuda_stream) == errors
