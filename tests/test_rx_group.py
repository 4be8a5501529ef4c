"""Grouping of received datagrams on the GPU (include/shorthair_rx.h: shorthair_rx_group_batch).

Expected values come from the rule of the header restated below datagram by datagram (rx_group_rule), for
the one large case from its numpy.cumsum form (proved equal to the sequential one on the small cases first),
and for the decodes from oracle/packets.py on the CPU oracle -- never from the library under test.
"""
import collections
import functools
import os
import subprocess

import numpy as np
import pytest

from oracle import packets as opk
from oracle import pyoracle as po
from tests.test_rx_list import CANARY, Guarded, deliveries, merge, orig_rec, rx_list_rule

MAXP = 512        # SHORTHAIR_RX_MAX_PACKETS
TILE = 256        # SHORTHAIR_RX_GROUP_TILE
TILE_PASS = 1024  # SHORTHAIR_RX_GROUP_TILE_PASS
SLOT_TILE = 16    # SHORTHAIR_RX_GROUP_SLOT_TILE
SLOT_PASS = 4096  # SHORTHAIR_RX_GROUP_SLOT_PASS
INCLUDE = os.path.join(os.path.dirname(__file__), "..", "include")
FIXTURE = os.path.join(os.path.dirname(__file__), "golden", "rx_datagrams.npz")
FIX_G, FIX_BACK = 64, 4  # the window the fixture is grouped in, from state 0
OUT_NAMES = ("state_out", "dg_class", "dg_slot", "pkt_first", "pkt_off", "pkt_len", "pkt_dg", "slot_group", "other",
             "summary")


# ---------------------------------------------------------------- the rule

def s_trunc(x, bits=7):
    """The low `bits` bits of x as a signed number: s7 of the header for bits = 7."""
    half = 1 << (bits - 1)
    return ((x & (2 * half - 1)) ^ half) - half


def expand(recent, partial, bits=7):
    """Counter<..>::ExpandFromTruncated (Counter.h:297-316) on an unwrapped `recent`."""
    return recent + s_trunc(partial - recent, bits)


def rx_group_rule(dg_off, dg_len, ring, ring_bytes, state, groups, back):
    """Steps 1 to 5 of the header, datagram by datagram: every output of the call as a dict of arrays."""
    n = len(dg_off)
    cls, slot = np.zeros(n, np.int32), np.full(n, -1, np.int32)
    recs = [[] for _ in range(groups)]  # per slot: (off, len, datagram)
    u = int(state)
    for i in range(n):
        off, ln = int(dg_off[i]), int(dg_len[i])
        if ln < 3 or off < 0 or off + ln > ring_bytes:  # step 1
            cls[i] = -1
            continue
        f = int(ring[off + 2])  # step 2
        pong, h = 0, 2
        if f & 0x80 and f & 1:
            if ln < 11:
                cls[i] = -1
                continue
            pong = 8
            if ln == 11:
                cls[i] = 2 + pong
                continue
            h = 11
            if int(ring[off + 11]) & 0x80:
                cls[i] = 1 + pong
                continue
        elif f & 0x80:
            cls[i] = 1
            continue
        if ln - h - 1 <= 2:  # step 3
            cls[i] = 3 + pong
            continue
        p = int(ring[off + h]) & 127
        u = expand(u, p)  # step 4
        assert u & 127 == p
        s = u - int(state) + back  # step 5
        if not 0 <= s < groups:
            cls[i] = 4 + pong
            continue
        cls[i], slot[i] = pong, s
        recs[s].append((off + h + 1, ln - h - 1, i))
    first = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.int32)
    total = int(first[-1])
    pkt_off, pkt_len, pkt_dg = np.zeros(n, np.int64), np.zeros(n, np.int32), np.full(n, -1, np.int32)
    flat = [r for rs in recs for r in rs]
    for j, (o, l, i) in enumerate(flat):
        pkt_off[j], pkt_len[j], pkt_dg[j] = o, l, i
    other = np.full(n, -1, np.int32)
    rest = np.flatnonzero(slot < 0)
    other[:len(rest)] = rest
    used = [s for s in range(groups) if recs[s]]
    good = cls >= 0
    summary = np.array([total, len(rest), used[0] if used else groups, used[-1] + 1 if used else 0, (cls == -1).sum(),
                        (good & ((cls & 7) == 4)).sum(), (cls >= 8).sum(), (good & ((cls & 7) == 3)).sum()], np.int32)
    return dict(state_out=np.array([u], np.int32), dg_class=cls, dg_slot=slot, pkt_first=first, pkt_off=pkt_off,
                pkt_len=pkt_len, pkt_dg=pkt_dg, slot_group=(int(state) - back + np.arange(groups)).astype(np.int32),
                other=other, summary=summary)


def rx_group_rule_cumsum(dg_off, dg_len, ring, ring_bytes, state, groups, back):
    """The same rule with the group number as a numpy.cumsum of the steps (for the one large case)."""
    n = len(dg_off)
    off, ln = np.asarray(dg_off, np.int64), np.asarray(dg_len, np.int64)
    ring = np.concatenate([np.asarray(ring, np.uint8), np.zeros(16, np.uint8)]).astype(np.int64)
    ok = (ln >= 3) & (off >= 0) & (off + ln <= ring_bytes)
    at = np.where(ok, off, 0)
    f = ring[at + 2]
    pong = ok & ((f & 0x81) == 0x81)
    ok &= ~(pong & (ln < 11))
    pong &= ok
    only = pong & (ln == 11)
    h = np.where(pong, 11, 2)
    b = np.where(pong & ~only, ring[at + np.where(pong & ~only, 11, 2)], f)
    oob = ok & ~only & ((b & 0x80) != 0)
    cand = ok & ~only & ~oob
    short = cand & (ln - h - 1 <= 2)
    data = cand & ~short
    p = b[data] & 127
    prev = np.concatenate([[int(state) & 127], p[:-1]])
    u = int(state) + np.cumsum(((((p - prev) & 127) ^ 64) - 64))
    s = u - int(state) + back
    inside = (s >= 0) & (s < groups)
    cls = np.full(n, -1, np.int64)
    cls[oob], cls[only], cls[short] = 1, 2, 3
    cls[data] = np.where(inside, 0, 4)
    cls[pong] += 8
    slot = np.full(n, -1, np.int64)
    slot[data] = np.where(inside, s, -1)
    binned = np.flatnonzero(slot >= 0)
    order = binned[np.argsort(slot[binned], kind="stable")]
    total = len(order)
    pkt_off, pkt_len, pkt_dg = np.zeros(n, np.int64), np.zeros(n, np.int32), np.full(n, -1, np.int32)
    pkt_off[:total], pkt_len[:total], pkt_dg[:total] = (off + h + 1)[order], (ln - h - 1)[order], order
    counts = np.bincount(slot[binned], minlength=groups)[:groups] if groups else np.zeros(0, np.int64)
    first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    other = np.full(n, -1, np.int32)
    rest = np.flatnonzero(slot < 0)
    other[:len(rest)] = rest
    used = np.flatnonzero(counts)
    summary = np.array([total, len(rest), used[0] if len(used) else groups, used[-1] + 1 if len(used) else 0,
                        (cls == -1).sum(), ((cls >= 0) & ((cls & 7) == 4)).sum(), (cls >= 8).sum(),
                        ((cls >= 0) & ((cls & 7) == 3)).sum()], np.int32)
    return dict(state_out=np.array([u[-1] if len(u) else int(state)], np.int32), dg_class=cls.astype(np.int32),
                dg_slot=slot.astype(np.int32), pkt_first=first, pkt_off=pkt_off, pkt_len=pkt_len, pkt_dg=pkt_dg,
                slot_group=(int(state) - back + np.arange(groups)).astype(np.int32), other=other, summary=summary)


# ---------------------------------------------------------------- building datagrams

PONG = bytes([0x81]) + bytes(range(1, 9))  # [f with bits 0x80 and 1][seen u32][count u32]


def seq(i):
    return bytes([i & 255, (i >> 8) & 255])


def dg_data(i, group, rec, pong=False):
    """[seq u16][pong prefix?][g & 0x7f][id][c][body]"""
    return seq(i) + (PONG if pong else b"") + bytes([group & 0x7F]) + bytes(rec)


def dg_oob(i, body, kind=0x80, pong=False):
    assert kind & 0x80 and (pong or not kind & 1)
    return seq(i) + (PONG if pong else b"") + bytes([kind]) + bytes(body)


def lay(rng, dgs, tail=0):
    """[datagram bytes] -> (ring, dg_off, dg_len), in a shuffled placement with gaps, the first 16 datagrams
    at offsets j (mod 8); `tail` bytes of gap behind the last one."""
    n = len(dgs)
    dg_off = np.zeros(n, np.int64)
    parts, pos = [], 0
    for j, i in enumerate(rng.permutation(n)):
        gap = (j - pos) % 8 if j < 16 else int(rng.integers(0, 8))
        parts.append(np.full(gap, 0xA5, np.uint8))
        pos += gap
        dg_off[i] = pos
        parts.append(np.frombuffer(dgs[i], np.uint8))
        pos += len(dgs[i])
    parts.append(np.full(tail, 0xA5, np.uint8))
    ring = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    return ring, dg_off, np.array([len(d) for d in dgs], np.int32)


def traffic(rng, n, group, per_group=9, noise=True):
    """n datagrams of a sender that interleaves: group g's last third falls among group g + 1's first
    datagrams. With `noise`, every other class appears among them."""
    dgs = []
    plan = []
    g = group
    while len(plan) < n:
        a = [(g, j) for j in range(per_group - per_group // 3, per_group)] if plan else []
        b = [(g + 1, j) for j in range(per_group - per_group // 3)]
        plan += merge(rng, a, b)
        g += 1
    shift = int(rng.integers(0, 40))
    for i, (g, j) in enumerate(plan[:n]):
        r = (7 * i + shift) % 40 if noise else 99  # every class once in 40 datagrams
        body = rng.integers(0, 256, size=int(rng.integers(1, 9)), dtype=np.uint8).tobytes()
        if r == 0:
            dgs.append(dg_oob(i, body))
        elif r == 1:
            dgs.append(seq(i) + PONG)
        elif r == 2:
            dgs.append(dg_oob(i, body, 0x9C, pong=True))
        elif r == 3:
            dgs.append(dg_data(i, g, bytes([j, j]) + body, pong=True))
        elif r == 4:
            dgs.append(dg_data(i, g + 77, bytes([j, j])))  # short: its group byte must not count
        elif r == 5:
            dgs.append(seq(i)[:int(rng.integers(0, 3))])
        elif r == 6:
            dgs.append(dg_data(i, g + 40 + int(rng.integers(0, 3)), bytes([j, j]) + body))  # a jump: out of window
        else:
            dgs.append(dg_data(i, g, bytes([j, j]) + body))
    return dgs


# ---------------------------------------------------------------- running on the GPU

@pytest.fixture(scope="module")
def sh():
    import torch
    import shorthair_amd
    assert shorthair_amd.cauchy_256_init() == 0
    torch.cuda.init()
    return shorthair_amd


def out_sizes(n, groups):
    return dict(state_out=4, dg_class=4 * n, dg_slot=4 * n, pkt_first=4 * (groups + 1), pkt_off=8 * n, pkt_len=4 * n,
                pkt_dg=4 * n, slot_group=4 * groups, other=4 * n, summary=32)


def guarded_outputs(n, groups, variant=0):
    """Every output array between canaries; variant 0: the least alignment the contract allows."""
    lo = variant == 0
    return {name: Guarded(size, (8 if name == "pkt_off" else 4 + 8 * (j % 2)) if lo else 0)
            for j, (name, size) in enumerate(out_sizes(n, groups).items())}


def run_group(sh, dg_off, dg_len, ring, state, groups, back, ring_bytes=None, variant=0, outs=None, alias=False):
    """Runs the call with every array and the scratch between canaries, checks the canaries and that the
    inputs are unchanged, and returns (rc, outputs as rx_group_rule's, the output buffers)."""
    import torch
    n = len(dg_off)
    lo = variant == 0
    ring_bytes = len(ring) if ring_bytes is None else ring_bytes
    d_off = Guarded(8 * n, 8 if lo else 0, np.asarray(dg_off, np.int64))
    d_len = Guarded(4 * n, 4 if lo else 0, np.asarray(dg_len, np.int32))
    d_ring = Guarded(len(ring), 5 if lo else 0, ring)
    d_state = Guarded(4, 12 if lo else 0, np.array([state], np.int32))
    outs = guarded_outputs(n, groups, variant) if outs is None else outs
    scratch = Guarded(sh.rx_group_scratch_bytes(n, groups), 8 if lo else 0)
    state_out = d_state if alias else outs["state_out"]
    rc = sh.lib.shorthair_rx_group_batch(n, groups, back, d_off.ptr, d_len.ptr, d_ring.ptr, ring_bytes, d_state.ptr,
                                         state_out.ptr, outs["dg_class"].ptr, outs["dg_slot"].ptr,
                                         outs["pkt_first"].ptr, outs["pkt_off"].ptr, outs["pkt_len"].ptr,
                                         outs["pkt_dg"].ptr, outs["slot_group"].ptr, outs["other"].ptr,
                                         outs["summary"].ptr, scratch.ptr, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    scratch.read(np.uint8)  # canaries
    assert d_off.unchanged() and d_len.unchanged() and d_ring.unchanged()
    got = {name: outs[name].read(np.int64 if name == "pkt_off" else np.int32) for name in OUT_NAMES}
    if alias:
        got["state_out"] = d_state.read(np.int32)
        assert (outs["state_out"].read(np.uint8) == CANARY).all()
    else:
        assert d_state.unchanged()
    return rc, got, outs


def sort_long_slots(res):
    """Records of a slot with more than MAXP records are in an unspecified order: sorted for comparison."""
    res = dict(res)
    first = res["pkt_first"]
    for s in np.flatnonzero(np.diff(first) > MAXP):
        a, b = int(first[s]), int(first[s + 1])
        order = a + np.argsort(res["pkt_dg"][a:b], kind="stable")
        for name in ("pkt_off", "pkt_len", "pkt_dg"):
            res[name] = res[name].copy()
            res[name][a:b] = res[name][order]
    return res


def assert_same(got, want, tag):
    got = sort_long_slots(got) if np.array_equal(got["pkt_first"], want["pkt_first"]) else got
    for name in ("summary", "state_out", "pkt_first", "dg_class", "dg_slot", "slot_group", "other", "pkt_dg", "pkt_off",
                 "pkt_len"):
        assert got[name].shape == want[name].shape, (tag, name)
        bad = np.flatnonzero(got[name] != want[name])
        assert not len(bad), (tag, name, bad[:6], got[name][bad[:6]], want[name][bad[:6]])


def check(sh, dg_off, dg_len, ring, state, groups, back, tag, ring_bytes=None, rule=rx_group_rule, variants=(0, 1),
          alias=False):
    """The call against the rule; a second call into the same buffers; the error counter."""
    rb = len(ring) if ring_bytes is None else ring_bytes
    want = rule(dg_off, dg_len, ring, rb, state, groups, back)
    sh.batch_errors()
    for variant in variants:
        rc, got, outs = run_group(sh, dg_off, dg_len, ring, state, groups, back, rb, variant, alias=alias)
        assert rc == 0
        assert_same(got, want, (tag, variant))
        assert sh.batch_errors() == want["summary"][4]
    # other inputs into the same output buffers: the same datagrams backwards, from another state
    state2 = state + 3
    off2, len2 = np.asarray(dg_off)[::-1].copy(), np.asarray(dg_len)[::-1].copy()
    want2 = rule(off2, len2, ring, rb, state2, groups, back)
    rc, got, _ = run_group(sh, off2, len2, ring, state2, groups, back, rb, variants[-1], outs=outs, alias=alias)
    assert rc == 0
    assert_same(got, want2, (tag, "second call"))
    assert sh.batch_errors() == want2["summary"][4]
    return want


# ---------------------------------------------------------------- CPU

def test_expansion_of_the_truncated_group():
    """The model's 7-bit expansion is the value congruent to the partial within [state - 64, state + 63]."""
    for state in range(256):
        for partial in range(128):
            near = [v for v in range(state - 64, state + 64) if v % 128 == partial]
            assert len(near) == 1
            assert expand(state, partial) % 256 == near[0] % 256, (state, partial)
            assert expand(state, partial) == near[0]
    # the worked examples of the Counter.h comment (an 8-bit truncation): recent, smaller -> expanded
    for recent, smaller, expanded in ((0x100, 0xFF, 0x0FF), (0x16F, 0x7F, 0x17F), (0x17F, 0x6F, 0x16F),
                                      (0x1FF, 0xA0, 0x1A0), (0x1FF, 0x01, 0x201)):
        assert expand(recent, smaller, bits=8) == expanded
    # the same five one bit narrower
    for recent, smaller, expanded in ((0x80, 0x7F, 0x7F), (0xB7, 0x3F, 0xBF), (0xBF, 0x37, 0xB7), (0xFF, 0x50, 0xD0),
                                      (0xFF, 0x01, 0x101)):
        assert expand(recent, smaller) == expanded


def test_rx_group_symbols_header_and_bindings(tmp_path):
    import shorthair_amd as sh
    for name in ("shorthair_rx_group_batch", "shorthair_rx_group_scratch_bytes"):
        assert name in sh.EXPORTED_SYMBOLS
        assert getattr(sh.lib, name) is not None
    assert callable(sh.rx_group_batch) and callable(sh.rx_group_scratch_bytes)
    assert (sh.RX_GROUP_TILE, sh.RX_GROUP_TILE_PASS, sh.RX_GROUP_SLOT_TILE, sh.RX_GROUP_SLOT_PASS) == \
        (TILE, TILE_PASS, SLOT_TILE, SLOT_PASS)
    text = open(os.path.join(INCLUDE, "shorthair_rx.h")).read()
    for name, value in (("TILE", TILE), ("TILE_PASS", TILE_PASS), ("SLOT_TILE", SLOT_TILE), ("SLOT_PASS", SLOT_PASS)):
        assert "#define SHORTHAIR_RX_GROUP_%s %d " % (name, value) in text, name
    # the header compiles as C, and a C caller links
    src = tmp_path / "caller.c"
    src.write_text('#include "shorthair_rx.h"\n'
                   "int main(void) {\n"
                   "    long long need = shorthair_rx_group_scratch_bytes(100, 4);\n"
                   "    int rc = shorthair_rx_group_batch(-1, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0);\n"
                   "    return need > 0 && rc == -1 ? 0 : 1;\n"
                   "}\n")
    libdir = os.path.dirname(sh.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", f"-I{INCLUDE}", str(src), "-o",
                    str(tmp_path / "caller"), f"-L{libdir}", "-lcauchy256", f"-Wl,-rpath,{libdir}"], check=True)


def test_rx_group_rejects_bad_arguments_without_gpu(capfd):
    """Every host-checked argument returns -1 before anything touches the GPU (there is none here: an
    initialisation attempt would print the library's "no HIP device" error)."""
    import shorthair_amd as sh
    f = sh.lib.shorthair_rx_group_batch
    p = 0x1000  # never dereferenced
    names = ["dg_off", "dg_len", "ring", "state_in", "state_out", "dg_class", "dg_slot", "pkt_first", "pkt_off",
             "pkt_len", "pkt_dg", "slot_group", "other", "summary", "scratch"]

    def call(datagrams=40, groups=4, back=1, ring_bytes=4096, **ptrs):
        a = {n: p for n in names}
        a.update(ptrs)
        return f(datagrams, groups, back, a["dg_off"], a["dg_len"], a["ring"], ring_bytes, a["state_in"],
                 a["state_out"], a["dg_class"], a["dg_slot"], a["pkt_first"], a["pkt_off"], a["pkt_len"], a["pkt_dg"],
                 a["slot_group"], a["other"], a["summary"], a["scratch"], None)

    assert call(groups=0, back=0) == 0                            # an empty window is fine, and no GPU work
    assert call(groups=0, back=0, datagrams=0, **{n: None for n in names}) == 0
    assert call(datagrams=-1) == -1 and call(groups=-1, back=0) == -1 and call(ring_bytes=-1) == -1
    assert call(back=-1) == -1 and call(back=5) == -1 and call(groups=0, back=1) == -1   # 0 <= back <= groups
    for n in ("dg_len", "state_in", "state_out", "dg_class", "dg_slot", "pkt_first", "pkt_len", "pkt_dg", "slot_group",
              "other", "summary"):
        for mis in (1, 2, 3):                                     # 4-byte alignment of the int arrays
            assert call(**{n: p + mis}) == -1, (n, mis)
            assert call(groups=0, back=0, **{n: p + mis}) == -1, (n, mis)
        assert call(groups=0, back=0, **{n: p + 4}) == 0
    for n in ("dg_off", "pkt_off", "scratch"):
        for mis in (1, 2, 4, 7, 12):                              # 8-byte alignment
            assert call(**{n: p + mis}) == -1, (n, mis)
            assert call(groups=0, back=0, **{n: p + mis}) == -1, (n, mis)
        assert call(groups=0, back=0, **{n: p + 8}) == 0
    for n in names:                                               # null pointers with groups > 0
        assert call(**{n: None}) == -1, n
    for n in ("state_in", "state_out", "pkt_first", "slot_group", "summary", "scratch"):
        assert call(datagrams=0, **{n: None}) == -1, n            # (these are written without datagrams too)
    assert call(groups=0, back=0, ring=p + 5) == 0                # the ring takes any address

    scr = sh.lib.shorthair_rx_group_scratch_bytes
    assert scr(-1, 0) == -1 and scr(0, -1) == -1
    steps = (0, 1, 2, 3, TILE - 1, TILE, TILE + 1, 4097, 2**31 - 1)
    sizes = [[scr(n, g) for g in steps] for n in steps]
    assert all(v > 0 for row in sizes for v in row)
    assert all(a <= b for row in sizes for a, b in zip(row, row[1:]))
    assert all(a <= b for r0, r1 in zip(sizes, sizes[1:]) for a, b in zip(r0, r1))
    with pytest.raises(ValueError):
        sh.rx_group_scratch_bytes(-1, 0)
    assert "libcauchy256" not in capfd.readouterr().err


def interleaved_groups(rng, ora, ks, m, B, first_group):
    """Groups of payloads sent the way a sender interleaves them -- group g's recovery datagrams fall among
    group g + 1's originals -- with loss. Returns (datagrams in arrival order, the group of each, per group
    the originals [(id, payload)] and recovery packets that arrived, in arrival order)."""
    runs, arrived = [], []
    for j, k in enumerate(ks):
        lens = [int(v) for v in rng.integers(1, B - 1, size=k)]  # (an empty payload makes a short datagram)
        lens[int(rng.integers(0, k))] = B - 2
        pk = [rng.integers(0, 256, size=v, dtype=np.uint8).tobytes() for v in lens]
        rec = opk.tx_group(ora, m, pk)
        e = int(rng.integers(0, m + 2)) if j % 5 else m + 1  # every fifth group loses too much
        lost = set(int(x) for x in rng.choice(k, size=min(e, k), replace=False))
        keep = sorted(int(y) for y in rng.choice(m, size=int(rng.integers(max(m - 1, 1), m + 1)), replace=False))
        runs.append(([(j, orig_rec(i, pk[i])) for i in range(k) if i not in lost], [(j, rec[y]) for y in keep]))
        arrived.append(([(i, pk[i]) for i in range(k) if i not in lost], [rec[y] for y in keep]))
    order = []
    for j in range(len(ks) + 1):
        order += merge(rng, runs[j][0] if j < len(ks) else [], runs[j - 1][1] if j else [])
    dgs = [dg_data(i, first_group + j, r) for i, (j, r) in enumerate(order)]
    return dgs, [j for j, _ in order], arrived


def test_rule_against_the_packet_oracle():
    """Datagrams from oracle/packets.py with the 3-byte prefix, interleaved and with loss: the records the
    rule puts into each slot are exactly the lists rx_group expects, and the listing rule on them decodes."""
    ora = po.oracle()
    rng = np.random.default_rng(5)
    m, B, first_group = 4, 24, 250  # the groups run across 255 -> 0
    ks = [int(v) for v in rng.integers(2, 21, size=12)]
    dgs, _, arrived = interleaved_groups(rng, ora, ks, m, B, first_group)
    ring, dg_off, dg_len = lay(rng, dgs)
    G, back = len(ks) + 2, 1
    res = rx_group_rule(dg_off, dg_len, ring, len(ring), first_group, G, back)
    assert res["summary"][0] == len(dgs) and res["summary"][1] == 0 and res["state_out"][0] == first_group + len(ks) - 1
    assert list(res["slot_group"]) == list(range(first_group - 1, first_group - 1 + G))
    lst = rx_list_rule(2, 20, m, B, G, len(dgs), res["pkt_first"], res["pkt_off"], res["pkt_len"], ring)
    for j, (orig, rec) in enumerate(arrived):
        s = j + back
        a, b = int(res["pkt_first"][s]), int(res["pkt_first"][s + 1])
        records = [ring[o:o + l].tobytes() for o, l in zip(res["pkt_off"][a:b], res["pkt_len"][a:b])]
        assert [(r[0], r[2:]) for r in records if r[0] <= r[1]] == orig, j
        assert [r for r in records if r[0] > r[1]] == rec, j
        assert (opk.rx_group(ora, orig, rec) is not None) == (lst["info"][s, 0] == 1), j


@functools.lru_cache(maxsize=None)
def fixture():
    """tests/golden/rx_datagrams.npz (tools/capture_datagrams.py): the datagrams the reference client's Recv
    was given, back to back as a ring, and the multiset of payloads its OnPacket delivered."""
    z = np.load(FIXTURE)
    ring, dg_len = z["dg_bytes"], z["dg_len"]
    dg_off = np.concatenate([[0], np.cumsum(dg_len)[:-1]]).astype(np.int64)
    ends = np.cumsum(z["pay_len"])
    pays = [z["pay_bytes"][e - l:e].tobytes() for e, l in zip(ends, z["pay_len"])]
    assert len(pays) == z["stats"][1] and len(dg_len) == z["stats"][3] - z["stats"][4]
    return ring, dg_off, dg_len, collections.Counter(pays), int(z["stats"][2])


def payloads_of(records, info, pkt_first, pkt_off, pkt_len, ring, recovered):
    """What a receiver delivers: the original payloads straight from the records, the k = 1 form from
    first_rec, and the recovered payloads of the listed slots."""
    got = [r[2:] for recs in records for r in recs if r[0] <= r[1]]
    for s in np.flatnonzero(info[:, 0] == 2):
        p = int(info[s, 7])
        got.append(ring[pkt_off[p] + 2:pkt_off[p] + pkt_len[p]].tobytes())
    return collections.Counter(got + [pay for rec in recovered for _, pay in rec])


def test_fixture_rule_delivers_what_the_reference_delivered():
    """The restated rules on the reference's own traffic: group, list per bucket, decode on the CPU oracle.
    The multiset of payloads is the one the reference's OnPacket delivered."""
    ring, dg_off, dg_len, want, n_oob = fixture()
    ora = po.oracle()
    n = len(dg_off)
    res = rx_group_rule(dg_off, dg_len, ring, len(ring), 0, FIX_G, FIX_BACK)
    assert res["summary"][4] == 0 and res["summary"][5] == 0 and res["summary"][7] == 0
    assert res["summary"][6] >= 1                                  # a statistics interval passed: pong prefixes
    assert ((res["dg_class"] & 7) == 1).sum() == n_oob >= 2       # the out-of-band sends
    assert res["summary"][0] + n_oob + (res["dg_class"] == 10).sum() == n
    args = (FIX_G, n, res["pkt_first"], res["pkt_off"], res["pkt_len"], ring)
    info = rx_list_rule(2, 255, 1, 8, *args)["info"]
    assert not (info[:, 0] == -1).any()
    buckets = sorted({(int(m), int(B)) for st, _, m, B in info[:, :4] if st in (1, 3)})
    assert buckets
    recovered, listed = [], 0
    for m, B in buckets:
        lst = rx_list_rule(2, 256 - m, m, B, *args)
        listed += int(lst["summary"][0])
        recovered += [deliveries(ora, B, ring, lst, slot) for slot in range(int(lst["summary"][0]))]
    assert listed == ((info[:, 0] == 1) | (info[:, 0] == 3)).sum()
    records = [[ring[o:o + l].tobytes() for o, l in zip(res["pkt_off"][a:b], res["pkt_len"][a:b])]
               for a, b in zip(res["pkt_first"][:-1], res["pkt_first"][1:])]
    got = payloads_of(records, info, res["pkt_first"], res["pkt_off"], res["pkt_len"], ring, recovered)
    assert got == want and sum(len(r) for r in recovered) > 0


def small_cases():
    """(tag, datagrams, state, groups, back) for the cases both forms of the rule are compared on."""
    rng = np.random.default_rng(3)
    out = [("traffic %d" % n, traffic(rng, n, 250 + n), 250 + n, 9, 3) for n in (0, 1, 65, 300)]
    out.append(("clean", traffic(rng, 200, 120, noise=False), 120, 40, 2))
    out.append(("narrow", traffic(rng, 200, 7), 7, 2, 0))
    return out


def test_cumsum_form_equals_the_sequential_model():
    rng = np.random.default_rng(4)
    for tag, dgs, state, groups, back in small_cases():
        ring, dg_off, dg_len = lay(rng, dgs)
        for rb in (len(ring), max(len(ring) - 5, 0)):
            a = rx_group_rule(dg_off, dg_len, ring, rb, state, groups, back)
            b = rx_group_rule_cumsum(dg_off, dg_len, ring, rb, state, groups, back)
            for name in OUT_NAMES:
                assert np.array_equal(a[name], b[name]), (tag, name)
    assert a["summary"][5] > 0 and a["summary"][4] > 0 and a["summary"][6] > 0 and a["summary"][7] > 0


# ---------------------------------------------------------------- GPU: counts, tiles, slots

@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 3])
def test_group_datagram_counts(sh, n):
    rng = np.random.default_rng(100 + n)
    dgs = traffic(rng, n, 251)
    ring, dg_off, dg_len = lay(rng, dgs)
    want = check(sh, dg_off, dg_len, ring, 251, 2 + n // 6, 2, n)
    assert n < 63 or (want["summary"][0] > n // 2 and want["summary"][4:].all())


@pytest.mark.gpu
def test_group_tile_pass_boundary(sh):
    """More tiles than the single workgroup takes per pass: 6-byte datagrams, about 240 per group, every
    seventh one belongs to the group before; an out-of-band datagram here and there."""
    n = TILE * TILE_PASS + TILE + 3
    i = np.arange(n)
    group = 100 + i // 240 - (i % 7 == 0)
    dg = np.zeros((n, 6), np.uint8)
    dg[:, 0], dg[:, 1], dg[:, 2], dg[:, 3], dg[:, 4], dg[:, 5] = i & 255, (i >> 8) & 255, group & 127, i % 200, i % 200, i % 251
    dg[i % 1013 == 5, 2] = 0x80
    dg_off, dg_len = (i * 6).astype(np.int64), np.full(n, 6, np.int32)
    G = n // 240 + 3
    check(sh, dg_off, dg_len, dg.reshape(-1), 100, G, 1, "pass", rule=rx_group_rule_cumsum, variants=(0,))


@pytest.mark.gpu
@pytest.mark.parametrize("groups", [1, SLOT_PASS - 1, SLOT_PASS, SLOT_PASS + 1])
def test_group_slot_counts(sh, groups):
    rng = np.random.default_rng(groups)
    dgs = traffic(rng, 40, 999, per_group=6)  # groups 1000, 1001, ...
    ring, dg_off, dg_len = lay(rng, dgs)
    for back in sorted({0, groups // 2, max(groups - 4, 0), groups}):  # the first slots, the middle, the last ones
        want = check(sh, dg_off, dg_len, ring, 1000, groups, back, (groups, back), variants=(0,))
        assert back == groups or want["summary"][0] > 0


# ---------------------------------------------------------------- GPU: steps of the group number

def data_run(partials):
    return [dg_data(i, p, bytes([i & 7, i & 7, 1, 2, 3])) for i, p in enumerate(partials)]


@pytest.mark.gpu
def test_group_steps(sh):
    rng = np.random.default_rng(7)
    cases = [
        ("+63 +64 +65", 0, [63, 127, 64, 127, 62, 2], 300, 150),          # +63, +64 = -64, +65 = -63, +63, +63, -60
        ("across 255 -> 0", 250, [122, 123, 124, 125, 126, 127, 0, 1, 2, 127, 3, 4], 16, 2),
        ("across 127 -> 0", 125, [125, 126, 127, 0, 1, 0, 127, 2], 16, 4),
        ("two groups interleaved", 40, [40, 41, 40, 41, 41, 40, 42, 41, 42, 42], 8, 1),
        ("three groups interleaved", 40, [40, 41, 42, 40, 42, 41, 40, 43, 41, 43, 42], 8, 1),
    ]
    for tag, state, partials, groups, back in cases:
        ring, dg_off, dg_len = lay(rng, data_run(partials))
        want = check(sh, dg_off, dg_len, ring, state, groups, back, tag)
        assert want["summary"][0] == len(partials), tag
    ring, dg_off, dg_len = lay(rng, data_run(cases[0][2]))
    want = rx_group_rule(dg_off, dg_len, ring, len(ring), 0, 300, 150)
    assert list(want["dg_slot"] - 150) == [63, -1, -64, -1, 62, 2]
    ring, dg_off, dg_len = lay(rng, data_run(cases[4][2]))
    steps = np.diff(rx_group_rule(dg_off, dg_len, ring, len(ring), 40, 8, 1)["dg_slot"])
    assert -1 in steps and -2 in steps
    # no data datagram at all: the state is unchanged; and d_state_out on top of d_state_in
    dgs = [dg_oob(0, b"abc"), seq(1) + PONG, dg_oob(2, b"xy", 0x9C, pong=True), dg_data(3, 9, bytes([1, 1])), seq(4)]
    ring, dg_off, dg_len = lay(rng, dgs)
    for alias in (False, True):
        want = check(sh, dg_off, dg_len, ring, 77, 4, 1, ("no data", alias), alias=alias)
        assert want["state_out"][0] == 77 and want["summary"][0] == 0 and want["summary"][2:4].tolist() == [4, 0]
    ring, dg_off, dg_len = lay(rng, traffic(rng, 300, 250))
    want = check(sh, dg_off, dg_len, ring, 250, 40, 2, "alias", alias=True)
    assert want["state_out"][0] > 270


# ---------------------------------------------------------------- GPU: classes, window, slot sizes, alignment

@pytest.mark.gpu
def test_group_classes(sh):
    rng = np.random.default_rng(8)
    rec = bytes([3, 3, 9, 9, 9])
    named = [
        ("data", dg_data(0, 5, rec), 0),
        ("plain out-of-band", dg_oob(1, b"hello"), 1),
        ("out-of-band, empty", dg_oob(2, b"", 0xFE), 1),
        ("pong only", seq(3) + PONG, 10),
        ("pong + out-of-band", dg_oob(4, b"oob", 0x80, pong=True), 9),
        ("pong + data", dg_data(5, 5, rec, pong=True), 8),
        ("pong + short", dg_data(6, 6, bytes([1, 1]), pong=True), 11),
        ("pong + one byte", seq(7) + PONG + bytes([6]), 11),
    ]
    named += [("truncated pong of %d" % ln, (seq(8) + PONG + bytes(4))[:ln], -1) for ln in range(3, 11)]
    named += [("len %d" % ln, (seq(9) + bytes([5]))[:ln], -1) for ln in range(3)]
    named += [("short data of %d" % ln, dg_data(10, 99, rec)[:ln], 3) for ln in (3, 4, 5)]
    named += [("data after the short ones", dg_data(11, 5, rec), 0), ("data of 6", dg_data(12, 5, rec)[:6], 0)]
    named += [("one byte past the ring", dg_data(13, 5, rec), -1), ("negative offset", dg_data(14, 5, rec), -1)]
    named += [("statistics byte without the flag", dg_data(15, 0x05, rec), 0), ("data again", dg_data(16, 6, rec), 0)]
    names = [c[0] for c in named]
    ring, dg_off, dg_len = lay(rng, [c[1] for c in named], tail=0)
    i = names.index("one byte past the ring")
    dg_off[i] = len(ring) - dg_len[i] + 1
    dg_off[names.index("negative offset")] = -1
    want = check(sh, dg_off, dg_len, ring, 5, 3, 1, "classes")
    assert [int(v) for v in want["dg_class"]] == [c[2] for c in named]
    n_bad = sum(1 for c in named if c[2] == -1)
    assert list(want["summary"]) == [6, len(named) - 6, 1, 3, n_bad, 0, 5, 5] and n_bad == 13
    assert want["state_out"][0] == 6  # the short datagrams' group byte moved nothing


@pytest.mark.gpu
def test_group_window(sh):
    rng = np.random.default_rng(9)
    # back = 0 with a backward step (slot -1); a step to slot == groups; both move the state
    partials = [50, 49, 50, 52, 53, 51, 50, 49, 52]
    ring, dg_off, dg_len = lay(rng, data_run(partials))
    want = check(sh, dg_off, dg_len, ring, 50, 3, 0, "window")
    assert list(want["dg_slot"]) == [0, -1, 0, 2, -1, 1, 0, -1, 2]
    assert list(want["dg_class"]) == [0, 4, 0, 0, 4, 0, 0, 4, 0] and want["summary"][5] == 3
    assert want["state_out"][0] == 52
    # a jump of +40 out of the window and what follows it
    ring, dg_off, dg_len = lay(rng, data_run([10, 50, 51, 11, 10, 12]))
    want = check(sh, dg_off, dg_len, ring, 10, 4, 1, "jump")
    assert list(want["dg_slot"]) == [1, -1, -1, 2, 1, 3]


def one_slot(rng, n, other=40):
    """n datagrams of group 21 scrambled among `other` of group 20 and 22. Every record is an original (id <=
    c), so the listing skips a group of them unless they are too many."""
    a = [(21, j) for j in range(n)]
    b = [(20 + 2 * int(rng.integers(0, 2)), j) for j in range(other)]
    return [dg_data(i, g, bytes([j & 127, 200, j >> 7])) for i, (g, j) in enumerate(merge(rng, a, b))]


@pytest.mark.gpu
def test_group_slot_spread_wide(sh):
    """A slot's records lie among thousands of other datagrams (the ordering kernel's other path), for slot
    sizes on both sides of a wave: the order is still exact."""
    rng = np.random.default_rng(12)
    for n in (2, 64, 65, 300, MAXP):
        ring, dg_off, dg_len = lay(rng, one_slot(rng, n, other=2600))
        want = check(sh, dg_off, dg_len, ring, 21, 3, 1, n, variants=(0,))
        mine = want["pkt_dg"][want["pkt_first"][1]:want["pkt_first"][2]]
        assert len(mine) == n and (n < 64 or mine[-1] - mine[0] >= 2048)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [MAXP, MAXP + 1, 1100])
def test_group_slot_sizes(sh, n):
    """Exactly 512 records: the order is exact. More: each exactly once, and the listing calls the group
    malformed."""
    import torch
    rng = np.random.default_rng(n)
    ring, dg_off, dg_len = lay(rng, one_slot(rng, n))
    want = check(sh, dg_off, dg_len, ring, 21, 3, 1, n, variants=(0,))
    assert want["pkt_first"][2] - want["pkt_first"][1] == n
    rc, got, _ = run_group(sh, dg_off, dg_len, ring, 21, 3, 1)
    a, b = int(got["pkt_first"][1]), int(got["pkt_first"][2])
    assert sorted(got["pkt_dg"][a:b]) == list(want["pkt_dg"][a:b])  # each exactly once
    if n <= MAXP:
        assert list(got["pkt_dg"][a:b]) == list(want["pkt_dg"][a:b])
    N = len(dg_off)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    cap = sh.rx_list_capacity(3, N, 8)
    info = torch.zeros((3, 8), dtype=torch.int32, device="cuda")
    t32 = lambda k: torch.zeros(k, dtype=torch.int32, device="cuda")  # noqa: E731
    t8 = lambda k: torch.zeros(k, dtype=torch.uint8, device="cuda")  # noqa: E731
    sh.batch_errors()
    assert sh.rx_list_batch(2, 8, 4, 16, 3, N, dev(got["pkt_first"]), dev(got["pkt_off"]), dev(got["pkt_len"]), dev(ring),
                            len(ring), info, t32(4), t32(3), torch.zeros(cap, dtype=torch.int64, device="cuda"), t32(cap),
                            t8(cap), t8(cap), t32(8), t8(sh.rx_list_scratch_bytes(3, N))) == 0
    status = info.cpu().numpy()[:, 0]
    assert (status[1] == -1) == (n > MAXP) and status[0] == 0 and status[2] == 0
    assert sh.batch_errors() == (n > MAXP)


@pytest.mark.gpu
def test_group_offsets_at_every_alignment(sh):
    rng = np.random.default_rng(11)
    dgs = traffic(rng, 48, 30)
    ring, dg_off, dg_len = lay(rng, dgs)
    assert set(int(v) % 8 for v in dg_off) == set(range(8))
    for shift in range(8):  # and the whole ring at every alignment
        ring2 = np.concatenate([np.full(shift, 0x5A, np.uint8), ring])
        check(sh, dg_off + shift, dg_len, ring2, 30, 8, 2, shift, variants=(0,))


# ---------------------------------------------------------------- GPU: the chain on the device

def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev_group(sh, ring, dg_off, dg_len, d_state_in, d_state_out, G, back):
    """shorthair_rx_group_batch on tensors; the outputs the later stages read, left on the device."""
    import torch
    n = len(dg_off)
    i32 = lambda k: torch.full((k,), -9, dtype=torch.int32, device="cuda")  # noqa: E731
    t = dict(pkt_first=i32(G + 1), pkt_off=torch.zeros(n, dtype=torch.int64, device="cuda"), pkt_len=i32(n), pkt_dg=i32(n),
             slot_group=i32(G), summary=i32(8), dg_class=i32(n), dg_slot=i32(n), other=i32(n))
    scratch = torch.full((sh.rx_group_scratch_bytes(n, G),), 0x77, dtype=torch.uint8, device="cuda")
    assert sh.rx_group_batch(n, G, back, dg_off, dg_len, ring, ring.numel(), d_state_in, d_state_out, t["dg_class"],
                             t["dg_slot"], t["pkt_first"], t["pkt_off"], t["pkt_len"], t["pkt_dg"], t["slot_group"],
                             t["other"], t["summary"], scratch) == 0
    return t


def dev_bucket(sh, ring, n, G, grp, kmin, kmax, m, B, decode=True):
    """list -> frame -> decode -> unframe for one (k range, m, B) bucket with upper bounds (route (b) of
    INTEGRATION 2f), nothing read on the host in between. Returns (d_info, per listed slot of the group call:
    the recovered [(id, payload)]). Without `decode`, the listing alone."""
    import torch
    i32 = lambda k: torch.full((k,), -9, dtype=torch.int32, device="cuda")  # noqa: E731
    u8 = lambda k: torch.full((k,), 0x77, dtype=torch.uint8, device="cuda")  # noqa: E731
    cap = sh.rx_list_capacity(G, n, kmax)
    info, lfirst, lslot = i32(G * 8).view(G, 8), i32(G + 1), i32(G)
    loff, llen, lraw, lrows, lsum = torch.zeros(cap, dtype=torch.int64, device="cuda"), i32(cap), u8(cap), u8(cap), i32(8)
    assert sh.rx_list_batch(kmin, kmax, m, B, G, n, grp["pkt_first"], grp["pkt_off"], grp["pkt_len"], ring, ring.numel(),
                            info, lfirst, lslot, loff, llen, lraw, lrows, lsum, u8(sh.rx_list_scratch_bytes(G, n))) == 0
    if not decode:
        return info.cpu().numpy(), {}
    blocks = torch.zeros((cap, B), dtype=torch.uint8, device="cuda")
    assert sh.frame_batch(B, cap, ring, ring.numel(), loff, llen, lraw, blocks) == 0
    emax = min(kmax, m)
    out, out_rows, count = u8(G * emax * B).view(G, emax, B), u8(G * emax).view(G, emax), i32(G)
    assert sh.decode_batch_out_var(kmax, m, B, G, lfirst, cap, blocks, lrows, out, out_rows, count) == 0
    slots = G * emax
    pcap = slots * (B - 2)
    pay, doff, dlen = u8(pcap), torch.zeros(slots + 1, dtype=torch.int64, device="cuda"), i32(slots)
    assert sh.unframe_batch(B, G, emax, emax, out, count, pay, pcap, doff, dlen,
                            u8(sh.unframe_scratch_bytes(G, emax))) == 0
    # only now the host looks
    errors = sh.batch_errors()
    n_listed = int(lsum.cpu()[0])
    assert errors == G - n_listed  # the empty tail slots of route (b), and nothing else
    ls, pay, doff, dlen, out_rows = (x.cpu().numpy() for x in (lslot, pay, doff, dlen, out_rows))
    recovered = {int(ls[q]): [(int(out_rows[q, i]), pay[doff[t]:doff[t] + dlen[t]].tobytes())
                              for i in range(emax) for t in [q * emax + i] if dlen[t] >= 0] for q in range(n_listed)}
    return info.cpu().numpy(), recovered


def slot_records(ring_host, grp, G):
    """Per slot of the group call: its records as bytes, from the CSR the call wrote."""
    pf, po_, pl = (grp[name].cpu().numpy() for name in ("pkt_first", "pkt_off", "pkt_len"))
    return [[ring_host[o:o + l].tobytes() for o, l in zip(po_[pf[s]:pf[s + 1]], pl[pf[s]:pf[s + 1]])] for s in range(G)]


def device_chain(sh, ring, dg_off, dg_len, d_state_in, d_state_out, G, back, kmax, m, B):
    """group -> list -> frame -> decode -> unframe on the device. Returns per unwrapped group: (originals
    [(id, payload)], recovered [(id, payload)] or None when the group was not listed)."""
    grp = dev_group(sh, ring, dg_off, dg_len, d_state_in, d_state_out, G, back)
    _, recovered = dev_bucket(sh, ring, len(dg_off), G, grp, 2, kmax, m, B)
    sg = grp["slot_group"].cpu().numpy()
    records = slot_records(ring.cpu().numpy(), grp, G)
    return {int(sg[s]): ([(r[0], r[2:]) for r in records[s] if r[0] <= r[1]], recovered.get(s)) for s in range(G)}


@pytest.mark.gpu
def test_group_chain_on_the_device(sh):
    """Raw datagrams of 24 interleaved groups with loss through group -> list -> frame -> decode -> unframe on
    the device: the payloads are the CPU oracle's. Then once more as a streaming receiver would: the batch
    cut in two in the middle of a group, the second half from the first's d_state_out with the unfinished
    groups' datagrams presented again."""
    import torch
    kmax, m, B, first_group = 28, 4, 136, 246
    assert sh.path(kmax, m, B) == "fixed"
    ora = po.oracle()
    rng = np.random.default_rng(24)
    ks = [int(v) for v in rng.integers(17, kmax + 1, size=24)]
    dgs, group_of, arrived = interleaved_groups(rng, ora, ks, m, B, first_group)
    want = {first_group + j: (orig, opk.rx_group(ora, orig, rec)) for j, (orig, rec) in enumerate(arrived)}
    assert sum(1 for v in want.values() if v[1] is not None) >= 12 and sum(1 for v in want.values() if v[1] is None) >= 4
    ring_h, dg_off, dg_len = lay(rng, dgs)
    ring = _dev(ring_h)
    sh.batch_errors()
    state = _dev(np.array([first_group], np.int32))
    state_out = torch.zeros(1, dtype=torch.int32, device="cuda")
    G, back = len(ks) + 3, 2
    got = device_chain(sh, ring, _dev(dg_off), _dev(dg_len), state, state_out, G, back, kmax, m, B)
    assert int(state_out.cpu()[0]) == first_group + len(ks) - 1
    for g, (orig, rec) in want.items():
        assert got[g][0] == orig, g
        assert got[g][1] == rec, g
    assert all(v == ([], None) for g, v in got.items() if g not in want)
    # the same traffic in two batches, cut in the middle of group 11's originals
    cut = min(i for i, j in enumerate(group_of) if j == 11) + 6
    assert group_of[cut] in (10, 11) and 11 in group_of[cut:] and 10 in group_of[cut:]
    first_half = device_chain(sh, ring, _dev(dg_off[:cut]), _dev(dg_len[:cut]), state, state_out, G, back, kmax, m, B)
    again = [i for i in range(cut) if group_of[i] >= 10]  # the unfinished groups' datagrams, in arrival order
    idx = np.array(again + list(range(cut, len(dgs))))
    second_half = device_chain(sh, ring, _dev(dg_off[idx]), _dev(dg_len[idx]), state_out, state_out, G, back, kmax, m, B)
    assert int(state_out.cpu()[0]) == first_group + len(ks) - 1
    for g, (orig, rec) in want.items():
        half = first_half if g < first_group + 10 else second_half
        assert half[g][0] == orig and half[g][1] == rec, g
    assert np.array_equal(ring.cpu().numpy(), ring_h)


@pytest.mark.gpu
def test_fixture_chain_delivers_what_the_reference_delivered(sh):
    """group -> list -> frame -> decode -> unframe on the reference's own traffic, with one extra listing call
    per (k range, m, B) bucket that d_info reports: the multiset of payloads is the reference's."""
    import torch
    ring_h, dg_off, dg_len, want, n_oob = fixture()
    n = len(dg_off)
    ring = _dev(ring_h)
    sh.batch_errors()
    state = torch.zeros(1, dtype=torch.int32, device="cuda")
    grp = dev_group(sh, ring, _dev(dg_off), _dev(dg_len), state, state, FIX_G, FIX_BACK)
    summary = grp["summary"].cpu().numpy()
    assert summary[4] == 0 and summary[5] == 0 and summary[1] == n - summary[0] and summary[6] >= 1
    assert ((grp["dg_class"].cpu().numpy() & 7) == 1).sum() == n_oob
    info, recovered = dev_bucket(sh, ring, n, FIX_G, grp, 2, 255, 1, 8, decode=False)  # which buckets are there?
    assert not recovered and not (info[:, 0] == -1).any()
    buckets = sorted({(int(m), int(B)) for st, _, m, B in info[:, :4] if st == 3})
    assert buckets
    found = []
    for m, B in buckets:
        bucket_info, rec = dev_bucket(sh, ring, n, FIX_G, grp, 2, 256 - m, m, B)
        assert sorted(rec) == [s for s in range(FIX_G) if bucket_info[s, 0] == 1]
        found += list(rec.values())
    assert len(found) == (info[:, 0] == 3).sum()
    pkt_first, pkt_off, pkt_len = (grp[name].cpu().numpy() for name in ("pkt_first", "pkt_off", "pkt_len"))
    got = payloads_of(slot_records(ring_h, grp, FIX_G), info, pkt_first, pkt_off, pkt_len, ring_h, found)
    assert got == want and sum(len(r) for r in found) > 0


# ---------------------------------------------------------------- GPU: the binding on tensors, in a graph

@pytest.mark.gpu
def test_group_python_binding_on_tensors_and_graph_replay(sh):
    """Two replays of a captured call, each on changed ring contents, give the rule's outputs."""
    import torch
    rng = np.random.default_rng(60)
    dgs = traffic(rng, 700, 90)
    ring, dg_off, dg_len = lay(rng, dgs)
    n, G, back, state = len(dgs), 90, 3, 90
    s = torch.cuda.Stream()
    d_ring, d_off, d_len, d_state = _dev(ring), _dev(dg_off), _dev(dg_len), _dev(np.array([state], np.int32))
    outs = guarded_outputs(n, G)
    t = {name: g.tensor(torch.int64 if name == "pkt_off" else torch.int32) for name, g in outs.items()}
    scratch = Guarded(sh.rx_group_scratch_bytes(n, G), 8)
    torch.cuda.synchronize()

    def run():
        assert sh.rx_group_batch(n, G, back, d_off, d_len, d_ring, d_ring.numel(), d_state, t["state_out"], t["dg_class"],
                                 t["dg_slot"], t["pkt_first"], t["pkt_off"], t["pkt_len"], t["pkt_dg"], t["slot_group"],
                                 t["other"], t["summary"], scratch.tensor(torch.uint8)) == 0

    def check_now(ring_now, tag):
        want = rx_group_rule(dg_off, dg_len, ring_now, len(ring_now), state, G, back)
        got = {name: outs[name].read(np.int64 if name == "pkt_off" else np.int32) for name in OUT_NAMES}
        scratch.read(np.uint8)
        assert_same(got, want, tag)
        assert np.array_equal(d_ring.cpu().numpy(), ring_now) and int(d_state.cpu()[0]) == state
        return want

    sh.batch_errors()
    with torch.cuda.stream(s):
        run()  # loads the kernels' code and creates the stream's error counter before the capture
    s.synchronize()
    malformed = int(check_now(ring, "eager")["summary"][4])
    # a captured graph replays on hardware queues of its own: the runtime needs its default of four
    queues = os.environ.get("GPU_MAX_HW_QUEUES")
    assert queues is None or int(queues) >= 4, queues
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        run()
    for rep in range(2):
        # other contents under the same offsets: every group byte moves by 3 + rep, some datagrams change class
        ring2 = ring.copy()
        for i in range(n):
            if dg_len[i] >= 3:
                b = int(ring2[dg_off[i] + 2])
                ring2[dg_off[i] + 2] = (b + 3 + rep) & 127 if not b & 0x80 else (0x81 if i % (5 + rep) == 0 else b)
        d_ring.copy_(torch.from_numpy(ring2))
        for v in t.values():
            v.fill_(5)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        want = check_now(ring2, rep)
        assert want["summary"][0] > 100
        malformed += int(want["summary"][4])
    assert sh.batch_errors(s.cuda_stream) == malformed
