"""Open code groups carried from one receive batch to the next on the GPU (include/shorthair_rx.h:
shorthair_rx_window_batch).

Expected values come from the rule of the header restated below slot by slot (rx_window_rule), from the
restated group and listing rules of tests/test_rx_group.py and tests/test_rx_list.py, and for the decodes
from oracle/packets.py on the CPU oracle -- never from the library under test.
"""
import collections
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from oracle import packets as opk
from oracle import pyoracle as po
from tests.test_rx_group import FIX_BACK, FIX_G, dev_group, fixture, interleaved_groups, lay, rx_group_rule
from tests.test_rx_list import CANARY, Guarded, deliveries, rx_list_rule

MAX_INFO = 4      # SHORTHAIR_RX_WINDOW_MAX_INFO
ALIGN = 16        # SHORTHAIR_RX_HOLD_ALIGN
SCAN_TILE = 16    # SHORTHAIR_RX_WINDOW_SCAN_TILE
SCAN_PASS = 4096  # SHORTHAIR_RX_WINDOW_SCAN_PASS
INFO = 8          # SHORTHAIR_RX_INFO_INTS
INCLUDE = os.path.join(os.path.dirname(__file__), "..", "include")
WIN_NAMES = ("base", "first", "off", "len", "dg", "done")
WIN_DTYPES = dict(base=np.int32, first=np.int32, off=np.int64, len=np.int32, dg=np.int32, done=np.uint8)


# ---------------------------------------------------------------- the rule

def s32(x):
    """x as a wrapped 32-bit signed value."""
    return ((int(x) + 2**31) % 2**32) - 2**31


def finished_flag(infos, so):
    """Step 2: f of old slot so from the listings' d_info arrays."""
    f = 0
    for info in infos:
        st, k, n_orig = int(info[so, 0]), int(info[so, 1]), int(info[so, 4])
        if st == -1:
            f = 2
        elif f == 0 and (st in (1, 2) or (st == 0 and k >= 1 and n_orig >= k)):
            f = 1
    return f


def span_ok(first, t, limit):
    a, b = int(first[t]), int(first[t + 1])
    return a >= 0 and b >= a and b <= limit


def rx_window_rule(groups, prev, infos, grp, datagrams, ring, ring_bytes, hold_off, hold_bytes, capacity, use_done=True):
    """Steps 1 to 8 of the header, slot by slot. prev: None or a dict of base, first, off, len, done and
    capacity; infos: d_info arrays [groups][8]; grp: the group call's pkt_first, pkt_off, pkt_len, pkt_dg and
    slot_group. Returns the next window's arrays, the summary, the error count and the ring afterwards.
    use_done = False switches the done codes off (every old slot counts as open): the guard of the tests."""
    copy = prev is not None and hold_bytes > 0
    ring = np.array(ring, np.uint8) if copy else ring
    Gb = int(grp["slot_group"][0])
    if prev is None:
        N, dp, dg = Gb, 0, 0
    else:
        P = int(prev["base"][0])
        d = s32(Gb - P)
        dp, dg, N = max(d, 0), max(-d, 0), s32(P + max(d, 0))
    newly = expired = ignored = below = malformed = 0
    if prev is not None:
        for so in range(groups):  # steps 2's counts over the old slots
            f = finished_flag(infos, so)
            old = int(prev["done"][so])
            d = (old if old else f) if use_done else 0
            newly += old == 0 and f == 1
            expired += so < dp and d == 0 and int(prev["first"][so + 1]) > int(prev["first"][so])
    for t in range(min(dg, groups)):  # step 3: below the window
        if span_ok(grp["pkt_first"], t, datagrams):
            below += int(grp["pkt_first"][t + 1]) - int(grp["pkt_first"][t])
    slots = []  # per next slot: [done, carried [(off, len)], new [(off, len, dg)], carried bytes]
    for s in range(groups):
        so, t = s + dp, s + dg
        done, carried, new, nbytes, bad = 0, [], [], 0, False
        if prev is not None and so < groups:
            old = int(prev["done"][so])
            done = (old if old else finished_flag(infos, so)) if use_done else 0
            if done == 0:
                if not span_ok(prev["first"], so, prev["capacity"]):
                    bad = True
                else:
                    for p in range(int(prev["first"][so]), int(prev["first"][so + 1])):
                        off, ln = int(prev["off"][p]), int(prev["len"][p])
                        if ln < 0 or off < 0 or off + ln > ring_bytes:  # step 4
                            bad = True
                            break
                        carried.append((off, ln))
        if t < groups:
            ok = span_ok(grp["pkt_first"], t, datagrams)
            a, b = int(grp["pkt_first"][t]), int(grp["pkt_first"][t + 1])
            if done == 0 and not bad:
                if ok:
                    new = [(int(grp["pkt_off"][q]), int(grp["pkt_len"][q]), int(grp["pkt_dg"][q])) for q in range(a, b)]
                else:
                    bad = True
            elif ok:
                ignored += b - a
        if bad:
            done, carried, new = 2, [], []
            malformed += 1
        if copy:
            nbytes = sum((ln + ALIGN - 1) // ALIGN * ALIGN for _, ln in carried)
        slots.append([done, carried, new, nbytes])
    # steps 5 to 7
    first = np.zeros(groups + 1, np.int32)
    off, ln, dgs = np.zeros(capacity, np.int64), np.zeros(capacity, np.int32), np.full(capacity, -1, np.int32)
    done_out = np.zeros(groups, np.uint8)
    total = used = n_carried = emptied = 0
    cut = False
    for s, (done, carried, new, nbytes) in enumerate(slots):
        n = len(carried) + len(new)
        if not cut and (total + n > capacity or (copy and used + nbytes > hold_bytes)):
            cut = True
        if cut and n:
            done, carried, new = 3, [], []
            emptied += 1
        elif not cut:
            at = hold_off + used
            for o, l in carried:
                if copy:
                    ring[at:at + l] = ring[o:o + l].copy()  # (the sources do not overlap the hold region)
                    off[total], ln[total] = at, l
                    at += (l + ALIGN - 1) // ALIGN * ALIGN
                else:
                    off[total], ln[total] = o, l
                total += 1
            n_carried += len(carried)
            used += nbytes
            for o, l, i in new:
                off[total], ln[total], dgs[total] = o, l, i
                total += 1
        done_out[s] = done
        first[s + 1] = total
    summary = np.array([total, n_carried, used, newly, expired, ignored, below, malformed + emptied], np.int64)
    return dict(base=np.array([N], np.int32), first=first, off=off, len=ln, dg=dgs, done=done_out, summary=summary,
                errors=malformed + emptied, ring=ring, capacity=capacity)


# ---------------------------------------------------------------- a receiver on the models

def records_of(win, ring):
    """Per slot: [(record bytes, dg)]."""
    f = win["first"]
    return [[(ring[o:o + l].tobytes(), int(i)) for o, l, i in zip(win["off"][f[s]:f[s + 1]], win["len"][f[s]:f[s + 1]],
                                                                  win["dg"][f[s]:f[s + 1]])] for s in range(len(f) - 1)]


def model_receiver(dg_off, dg_len, ring, cuts, G, back, state=0, use_done=True, capacity=None, hold=False):
    """The datagrams in batches cut at `cuts`, through the restated group, window and listing rules and the
    CPU oracle. Returns (per unwrapped group the delivered [(id or None, payload)], the sum of the window
    summaries, the largest record count of a window). With `hold`, carried records move between two hold
    regions behind the ring, and the previous region is wiped after every window call."""
    ora = po.oracle()
    n_all = len(dg_off)
    capacity = n_all if capacity is None else capacity
    ring_bytes = len(ring)
    hold_bytes = 0
    if hold:
        hold_bytes = (int(np.sum((np.asarray(dg_len, np.int64) + ALIGN - 1) // ALIGN * ALIGN)) + ALIGN)
        ring = np.concatenate([ring, np.full(2 * hold_bytes + 5, 0xEE, np.uint8)])
    got = collections.defaultdict(list)
    sums, prev, infos, peak = np.zeros(8, np.int64), None, [], 0
    bounds = [0] + sorted(cuts) + [n_all]
    for i, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
        grp = rx_group_rule(dg_off[a:b], dg_len[a:b], ring, ring_bytes, state, G, back)
        state = int(grp["state_out"][0])
        hold_off = ring_bytes + 5 + (i & 1) * hold_bytes
        win = rx_window_rule(G, prev, infos, grp, b - a, ring, len(ring), hold_off if hold else 0, hold_bytes, capacity,
                             use_done)
        assert win["errors"] == 0
        if hold:
            ring = win["ring"]
            other = ring_bytes + 5 + ((i + 1) & 1) * hold_bytes
            ring[other:other + hold_bytes] = 0xEE  # the previous hold region is free again
        sums += win["summary"]
        peak = max(peak, int(win["summary"][0]))
        base = int(win["base"][0])
        for s, recs in enumerate(records_of(win, ring)):  # the originals of this batch, as OnData delivers them
            got[base + s] += [(r[0], r[2:]) for r, dg in recs if dg >= 0 and r[0] <= r[1]]
        args = (G, capacity, win["first"], win["off"], win["len"], ring)
        probe = rx_list_rule(2, 255, 1, 8, *args)["info"]
        for s in np.flatnonzero(probe[:, 0] == 2):  # the k == 1 form
            p = int(probe[s, 7])
            got[base + int(s)].append((0, ring[win["off"][p] + 2:win["off"][p] + win["len"][p]].tobytes()))
        buckets = sorted({(int(m), int(B)) for st, _, m, B in probe[:, :4] if st in (1, 3)})
        assert len(buckets) <= MAX_INFO
        infos = []
        for m, B in buckets:
            lst = rx_list_rule(2, 256 - m, m, B, *args)
            infos.append(lst["info"])
            for slot in range(int(lst["summary"][0])):
                got[base + int(lst["slot_group"][slot])] += deliveries(ora, B, ring, lst, slot)
        infos = infos or [probe]
        prev = win
    return got, sums, peak


def multiset(got):
    return collections.Counter(pay for v in got.values() for _, pay in v)


# ---------------------------------------------------------------- CPU

def test_rx_window_symbols_header_and_bindings(tmp_path):
    import shorthair_amd as sh
    for name in ("shorthair_rx_window_batch", "shorthair_rx_window_scratch_bytes"):
        assert name in sh.EXPORTED_SYMBOLS
        assert getattr(sh.lib, name) is not None
    assert callable(sh.rx_window_batch) and callable(sh.rx_window_scratch_bytes) and callable(sh.RxWindow)
    assert (sh.RX_WINDOW_MAX_INFO, sh.RX_HOLD_ALIGN, sh.RX_WINDOW_SCAN_TILE, sh.RX_WINDOW_SCAN_PASS) == \
        (MAX_INFO, ALIGN, SCAN_TILE, SCAN_PASS)
    text = open(os.path.join(INCLUDE, "shorthair_rx.h")).read()
    for name, value in (("WINDOW_MAX_INFO", MAX_INFO), ("HOLD_ALIGN", ALIGN), ("WINDOW_SCAN_TILE", SCAN_TILE),
                        ("WINDOW_SCAN_PASS", SCAN_PASS)):
        assert "#define SHORTHAIR_RX_%s %d " % (name, value) in text, name
    assert ctypes.sizeof(sh.RxWindowStruct) == 56
    # the header compiles as C, and a C caller links; the struct has the layout the binding assumes
    src = tmp_path / "caller.c"
    src.write_text('#include <stddef.h>\n#include "shorthair_rx.h"\n'
                   "int main(void) {\n"
                   "    ShorthairRxWindow w = {0, 0, 0, 0, 0, 0, 0};\n"
                   "    long long need = shorthair_rx_window_scratch_bytes(100, 4);\n"
                   "    int rc = shorthair_rx_window_batch(-1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, &w, 0, 0, 0);\n"
                   "    return need > 0 && rc == -1 && sizeof w == 56 && offsetof(ShorthairRxWindow, capacity) == 48 ? 0 : 1;\n"
                   "}\n")
    libdir = os.path.dirname(sh.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", f"-I{INCLUDE}", str(src), "-o",
                    str(tmp_path / "caller"), f"-L{libdir}", "-lcauchy256", f"-Wl,-rpath,{libdir}"], check=True)
    subprocess.run([str(tmp_path / "caller")], check=True)


def test_rx_window_rejects_bad_arguments_without_gpu(capfd):
    """Every host-checked argument returns -1 before anything touches the GPU (there is none here: an
    initialisation attempt would print the library's "no HIP device" error)."""
    import shorthair_amd as sh
    f = sh.lib.shorthair_rx_window_batch
    p = 0x1000  # never dereferenced
    names = ["pkt_first", "pkt_off", "pkt_len", "pkt_dg", "slot_group", "ring", "summary", "scratch"]

    def window(at, capacity=64, **ptrs):
        a = {n: at + 0x100 * j for j, n in enumerate(WIN_NAMES)}
        a.update(ptrs)
        return sh.RxWindowStruct(*[a[n] for n in WIN_NAMES], capacity)

    def call(groups=4, prev="yes", n_info=1, infos="yes", datagrams=40, ring_bytes=4096, hold_off=1024, hold_bytes=512,
             nxt="yes", **ptrs):
        a = {n: p for n in names}
        a.update(ptrs)
        prev = window(0x10000) if prev == "yes" else prev
        nxt = window(0x20000) if nxt == "yes" else nxt
        arr = (ctypes.c_void_p * 4)(*([0x30000 + 0x100 * j for j in range(4)] if infos == "yes" else infos or ()))
        return f(groups, None if prev is None else ctypes.addressof(prev), n_info,
                 None if infos is None else ctypes.addressof(arr), datagrams, a["pkt_first"], a["pkt_off"], a["pkt_len"],
                 a["pkt_dg"], a["slot_group"], a["ring"], ring_bytes, hold_off, hold_bytes,
                 None if nxt is None else ctypes.addressof(nxt), a["summary"], a["scratch"], None)

    assert call(groups=0) == 0                                    # an empty window is fine, and no GPU work
    assert call(groups=0, prev=None, n_info=0, infos=None, datagrams=0, **{n: None for n in names}) == 0
    assert call(groups=-1) == -1 and call(datagrams=-1) == -1
    assert call(nxt=window(0x20000, capacity=-1)) == -1 and call(prev=window(0x10000, capacity=-1)) == -1
    assert call(nxt=None) == -1 and call(groups=0, nxt=None) == -1
    for n_info in (-1, 5):
        assert call(n_info=n_info) == -1 and call(groups=0, n_info=n_info) == -1   # 0 <= n_info <= 4
    assert call(groups=0, n_info=0) == 0 and call(groups=0, n_info=4) == 0
    assert call(prev=None, n_info=1) == -1 and call(groups=0, prev=None, n_info=1) == -1  # a fresh receiver has none
    assert call(n_info=2, infos=None) == -1
    assert call(ring_bytes=-1, hold_off=0, hold_bytes=0) == -1 and call(hold_off=-1) == -1 and call(hold_bytes=-1) == -1
    assert call(groups=0, hold_off=4096 - 512) == 0 and call(groups=0, hold_off=4096 - 511) == -1  # inside the ring
    assert call(groups=0, hold_off=2**62, hold_bytes=2**62) == -1
    for which in ("prev", "nxt"):
        at = 0x10000 if which == "prev" else 0x20000
        for j, n in enumerate(WIN_NAMES):
            here = at + 0x100 * j
            if n != "done":
                for mis in ((1, 2, 3) if n != "off" else (1, 2, 4, 7, 12)):  # 4-byte and 8-byte alignment
                    assert call(**{which: window(at, **{n: here + mis})}) == -1, (which, n, mis)
                    assert call(groups=0, **{which: window(at, **{n: here + mis})}) == -1, (which, n, mis)
            assert call(groups=0, **{which: window(at, **{n: here + 8})}) == 0
            assert call(**{which: window(at, **{n: None})}) == -1, (which, n)  # null with groups > 0
            if n in ("base", "first", "done"):
                assert call(**{which: window(at, capacity=0, **{n: None})}) == -1, (which, n)
        assert call(groups=0, **{which: window(at, done=at + 0x501)}) == 0  # the done bytes take any address
    for j in range(4):
        for mis in (1, 2, 3):
            infos = [0x30000 + 0x100 * q + (mis if q == j else 0) for q in range(4)]
            assert call(n_info=j + 1, infos=infos) == -1 and call(groups=0, n_info=j + 1, infos=infos) == -1
            assert call(groups=0, n_info=j, infos=infos) == 0    # (only the first n_info are looked at)
        infos = [0x30000 + 0x100 * q if q != j else None for q in range(4)]
        assert call(n_info=4, infos=infos) == -1
    for n in ("pkt_first", "pkt_len", "pkt_dg", "slot_group"):
        for mis in (1, 2, 3):
            assert call(**{n: p + mis}) == -1 and call(groups=0, **{n: p + mis}) == -1, (n, mis)
        assert call(groups=0, **{n: p + 4}) == 0
    for n in ("pkt_off", "summary", "scratch"):
        for mis in (1, 2, 4, 7, 12):
            assert call(**{n: p + mis}) == -1 and call(groups=0, **{n: p + mis}) == -1, (n, mis)
        assert call(groups=0, **{n: p + 8}) == 0
    for n in names:                                               # null pointers with groups > 0
        assert call(**{n: None}) == -1, n
    for n in ("pkt_first", "slot_group", "summary", "scratch"):
        assert call(datagrams=0, **{n: None}) == -1, n
    assert call(groups=0, ring=p + 5) == 0                        # the ring takes any address
    # prev and next share no array
    for a in WIN_NAMES:
        for b in WIN_NAMES:
            shared = 0x40000
            assert call(groups=0, prev=window(0x10000, **{a: shared}), nxt=window(0x20000, **{b: shared})) == -1, (a, b)
    w = window(0x10000)
    assert call(groups=0, prev=w, nxt=w) == -1

    scr = sh.lib.shorthair_rx_window_scratch_bytes
    assert scr(-1, 0) == -1 and scr(0, -1) == -1
    steps = (0, 1, 2, 3, 255, 256, 257, 4097, 2**31 - 1)
    sizes = [[scr(g, n) for n in steps] for g in steps]
    assert all(v > 0 for row in sizes for v in row)
    assert all(a <= b for row in sizes for a, b in zip(row, row[1:]))
    assert all(a <= b for r0, r1 in zip(sizes, sizes[1:]) for a, b in zip(r0, r1))
    with pytest.raises(ValueError):
        sh.rx_window_scratch_bytes(-1, 0)
    assert "libcauchy256" not in capfd.readouterr().err


def batches_of(n, size):
    return list(range(size, n, size))


@functools.lru_cache(maxsize=None)
def fixture_in_batches(size, G, back, use_done=True, hold=False):
    ring, dg_off, dg_len, want, _ = fixture()
    got, sums, peak = model_receiver(dg_off, dg_len, ring, batches_of(len(dg_off), size), G, back, use_done=use_done,
                                     hold=hold)
    return multiset(got), sums, peak


@pytest.mark.parametrize("window", [(FIX_G, FIX_BACK), (8, 1)], ids=lambda w: "G%d_back%d" % w)
@pytest.mark.parametrize("size", [1983, 500, 97, 13, 1])
def test_fixture_in_batches_delivers_what_the_reference_delivered(size, window):
    """The reference client's 1,983 datagrams cut into batches, through the restated group, window and listing
    rules and the CPU oracle: the delivered multiset is exactly what the reference's OnPacket delivered.

    One combination cannot deliver everything: all 1,983 datagrams in one batch span more groups than a window
    of 8 slots, so the group call itself classes the later ones as out of window (its kind 4) before the window
    call sees them. There the expected multiset is exactly what the groups that the 8 slots admit deliver:
    groups -1 .. 6 from state 0 with back 1, taken from the whole batch in the 64-slot window."""
    want = fixture()[3]
    got, sums, _ = fixture_in_batches(size, *window)
    assert sum(want.values()) == 1016
    if size == 1983 and window[0] == 8:
        ring, dg_off, dg_len = fixture()[:3]
        assert rx_group_rule(dg_off, dg_len, ring, len(ring), 0, *window)["summary"][5] > 0
        per_group, _, _ = model_receiver(dg_off, dg_len, ring, [], FIX_G, FIX_BACK)
        assert multiset(per_group) == want
        admitted = multiset({g: v for g, v in per_group.items() if -window[1] <= g < window[0] - window[1]})
        assert got == admitted and 0 < sum(admitted.values()) < 1016 and not admitted - want
        return
    assert got == want, (sum(got.values()), sum(want.values()))
    assert sums[4] == 0 and sums[6] == 0 and sums[7] == 0  # nothing expired, fell below the window or was malformed
    if size == 97:
        assert (sums[1], sums[5], sums[3]) == (775, 678, 13)
    if size == 1983:
        assert sums[1] == 0 and sums[5] == 0


def test_fixture_needs_the_done_codes_and_survives_the_hold_copy():
    """With the done codes switched off in the model the late recovery datagrams of a decoded group form a
    group of their own and it is delivered twice: the fixture exercises step 3. With the hold copy switched
    on and the previous hold region wiped after every call, the multiset is still the reference's."""
    want = fixture()[3]
    got, sums, _ = fixture_in_batches(97, FIX_G, FIX_BACK, use_done=False)
    assert got != want and sum(got.values()) > sum(want.values())
    got, sums, peak = fixture_in_batches(97, FIX_G, FIX_BACK, hold=True)
    assert got == want and sums[1] == 775 and sums[2] > 775 * 16 and peak < 1024


def test_cut_invariance_on_synthetic_traffic():
    """Interleaved groups with loss, cut at 5 random places: every group delivers what the single batch
    delivers, and that is the packet oracle's."""
    ora = po.oracle()
    rng = np.random.default_rng(24)
    m, B, first_group = 4, 136, 246
    ks = [int(v) for v in rng.integers(17, 29, size=24)]
    dgs, group_of, arrived = interleaved_groups(rng, ora, ks, m, B, first_group)
    ring, dg_off, dg_len = lay(rng, dgs)
    G, back = len(ks) + 3, 2
    whole, _, _ = model_receiver(dg_off, dg_len, ring, [], G, back, state=first_group)
    for j, (orig, rec) in enumerate(arrived):
        assert sorted(whole[first_group + j]) == sorted(orig + (opk.rx_group(ora, orig, rec) or [])), j
    carried = 0
    for trial in range(4):
        cuts = sorted(int(v) for v in rng.choice(np.arange(1, len(dgs)), size=5, replace=False))
        got, sums, _ = model_receiver(dg_off, dg_len, ring, cuts, G, back, state=first_group, hold=trial % 2 == 1)
        for g in set(whole) | set(got):
            assert sorted(got[g]) == sorted(whole[g]), (trial, g)
        carried += int(sums[1])
    assert carried > 0


# ---------------------------------------------------------------- running on the GPU

@pytest.fixture(scope="module")
def sh():
    import torch
    import shorthair_amd
    assert shorthair_amd.cauchy_256_init() == 0
    torch.cuda.init()
    return shorthair_amd


def win_sizes(groups, capacity):
    return dict(base=4, first=4 * (groups + 1), off=8 * capacity, len=4 * capacity, dg=4 * capacity, done=groups)


def guarded_window(groups, capacity, variant, data=None):
    """A window's six arrays between canaries; variant 0: the least alignment the contract allows (4 for ints,
    8 for off, odd for done), 1: 16 bytes."""
    lo = variant == 0
    mis = dict(base=12, first=4, off=8, len=12, dg=4, done=3)
    return {name: Guarded(size, mis[name] if lo else 0,
                          None if data is None else np.asarray(data[name], WIN_DTYPES[name]))
            for name, size in win_sizes(groups, capacity).items()}


def struct_of(sh, guards, capacity):
    return sh.RxWindowStruct(*[guards[name].ptr for name in WIN_NAMES], capacity)


def run_window(sh, c, hold_bytes, capacity=None, variant=0, outs=None, fresh=False, n_info=None):
    """Runs the call on case `c` with every array and the scratch between canaries, checks the canaries and
    that the inputs are unchanged, and returns (rc, outputs as rx_window_rule's, the output buffers)."""
    import torch
    lo = variant == 0
    groups, n = c["groups"], c["datagrams"]
    capacity = c["capacity"] if capacity is None else capacity
    ring, hold_off = ring_of(c, hold_bytes)
    prev = None if fresh else c["prev"]
    infos = [] if fresh else c["infos"][:len(c["infos"]) if n_info is None else n_info]
    d_prev = None if prev is None else guarded_window(groups, prev["capacity"], variant, prev)
    d_infos = [Guarded(4 * INFO * groups, 4 if lo else 0, info) for info in infos]
    grp = c["grp"]
    d_grp = dict(pkt_first=Guarded(4 * (groups + 1), 12 if lo else 0, np.asarray(grp["pkt_first"], np.int32)),
                 pkt_off=Guarded(8 * n, 8 if lo else 0, np.asarray(grp["pkt_off"], np.int64)),
                 pkt_len=Guarded(4 * n, 4 if lo else 0, np.asarray(grp["pkt_len"], np.int32)),
                 pkt_dg=Guarded(4 * n, 12 if lo else 0, np.asarray(grp["pkt_dg"], np.int32)),
                 slot_group=Guarded(4 * groups, 4 if lo else 0, np.asarray(grp["slot_group"], np.int32)))
    d_ring = Guarded(len(ring), 5 if lo else 0, ring)
    if outs is None:
        outs = guarded_window(groups, capacity, variant)
        outs["summary"] = Guarded(64, 8 if lo else 0)
    pcap = 0 if prev is None else prev["capacity"]
    scratch = Guarded(sh.rx_window_scratch_bytes(groups, max(capacity, pcap)), 8 if lo else 0)
    s_prev = None if prev is None else struct_of(sh, d_prev, pcap)
    s_next = struct_of(sh, outs, capacity)
    arr = (ctypes.c_void_p * MAX_INFO)(*[g.ptr for g in d_infos])
    rc = sh.lib.shorthair_rx_window_batch(groups, None if s_prev is None else ctypes.addressof(s_prev), len(infos),
                                          ctypes.addressof(arr), n, d_grp["pkt_first"].ptr, d_grp["pkt_off"].ptr,
                                          d_grp["pkt_len"].ptr, d_grp["pkt_dg"].ptr, d_grp["slot_group"].ptr, d_ring.ptr,
                                          len(ring), hold_off, hold_bytes, ctypes.addressof(s_next), outs["summary"].ptr,
                                          scratch.ptr, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    scratch.read(np.uint8)  # canaries
    assert all(g.unchanged() for g in d_grp.values()) and all(g.unchanged() for g in d_infos)
    assert d_prev is None or all(g.unchanged() for g in d_prev.values())
    got = {name: outs[name].read(WIN_DTYPES[name]) for name in WIN_NAMES}
    got["summary"] = outs["summary"].read(np.int64)
    got["ring"] = d_ring.read(np.uint8)
    return rc, got, outs


def assert_same(got, want, tag):
    for name in ("summary", "base", "done", "first", "dg", "len", "off", "ring"):
        assert got[name].shape == want[name].shape, (tag, name)
        bad = np.flatnonzero(got[name] != want[name])
        assert not len(bad), (tag, name, bad[:6], got[name][bad[:6]], want[name][bad[:6]])


def want_of(c, hold_bytes, capacity=None, fresh=False, n_info=None):
    ring, hold_off = ring_of(c, hold_bytes)
    infos = [] if fresh else c["infos"][:len(c["infos"]) if n_info is None else n_info]
    want = rx_window_rule(c["groups"], None if fresh else c["prev"], infos, c["grp"], c["datagrams"], ring, len(ring),
                          hold_off, hold_bytes, c["capacity"] if capacity is None else capacity)
    want["ring"] = np.asarray(want["ring"])
    return want


def check(sh, c, tag, hold_bytes=None, capacity=None, variants=(0, 1), n_info=None):
    """The call against the rule at both alignment variants, the error counter, and a second call -- a fresh
    receiver on the same new records -- into the same output buffers."""
    hold_bytes = c["hold_bytes"] if hold_bytes is None else hold_bytes
    want = want_of(c, hold_bytes, capacity, n_info=n_info)
    sh.batch_errors()
    for variant in variants:
        rc, got, outs = run_window(sh, c, hold_bytes, capacity, variant, n_info=n_info)
        assert rc == 0
        assert_same(got, want, (tag, variant))
        assert sh.batch_errors() == want["errors"]
    want2 = want_of(c, hold_bytes, capacity, fresh=True)
    rc, got, _ = run_window(sh, c, hold_bytes, capacity, variants[-1], outs=outs, fresh=True)
    assert rc == 0
    assert_same(got, want2, (tag, "second call"))
    assert sh.batch_errors() == want2["errors"]
    return want


# ---------------------------------------------------------------- building cases

LENS = (2, 3, 7, 8, 9, 15, 16, 17, 139)  # (139 = B + 3 for B = 136)
FILL = 0xB7


def ring_of(c, hold_bytes):
    """[the records' region][16..31 bytes][the hold region, at c["hold_mis"] (mod 16)][48 bytes]; everything
    outside the records is FILL, so a stray write shows."""
    src = c["src"]
    gap = 16 + (c["hold_mis"] - len(src)) % 16
    ring = np.concatenate([src, np.full(gap + hold_bytes + 48, FILL, np.uint8)])
    return ring, len(src) + gap


def make_case(rng, groups, shift=0, n_info=1, prev_counts=None, new_counts=None, lens=LENS, P=1000, hold_mis=0,
              aligned_sources=False):
    """A previous window at base P with every done code and every status in its listings' d_info, and a group
    call's outputs at base P + shift. The records lie scattered in one region at every alignment."""
    prev_counts = rng.integers(0, 4, size=groups) if prev_counts is None else np.asarray(prev_counts)
    new_counts = rng.integers(0, 4, size=groups) if new_counts is None else np.asarray(new_counts)
    n_prev, n_new = int(prev_counts.sum()), int(new_counts.sum())
    rec_len = np.concatenate([rng.choice(lens, size=n_prev), rng.choice(lens, size=n_new)]).astype(np.int32)
    if aligned_sources:  # record j: length lens[j % len(lens)] at alignment (j // len(lens)) % 16
        rec_len = np.array([lens[j % len(lens)] for j in range(n_prev + n_new)], np.int32)
    rec_off = np.zeros(n_prev + n_new, np.int64)
    parts, pos = [], 0
    for j in (np.arange(n_prev + n_new) if aligned_sources else rng.permutation(n_prev + n_new)):
        gap = ((j // len(lens)) % 16 - pos) % 16 if aligned_sources else int(rng.integers(0, 16))
        parts.append(np.full(gap, FILL, np.uint8))
        pos += gap
        rec_off[j] = pos
        parts.append(rng.integers(0, 256, size=int(rec_len[j]), dtype=np.uint8))
        pos += int(rec_len[j])
    src = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    pcap = n_prev + 3
    prev = dict(base=np.array([s32(P)], np.int32),
                first=np.concatenate([[0], np.cumsum(prev_counts)]).astype(np.int32),
                off=np.concatenate([rec_off[:n_prev], np.zeros(3, np.int64)]),
                len=np.concatenate([rec_len[:n_prev], np.zeros(3, np.int32)]),
                dg=np.full(pcap, -1, np.int32), done=rng.choice([0, 0, 0, 0, 1, 2, 3], size=groups).astype(np.uint8),
                capacity=pcap)
    infos = []
    for _ in range(n_info):
        info = rng.integers(-3, 9, size=(groups, INFO)).astype(np.int32)
        info[:, 0] = rng.choice([-1, 0, 0, 0, 0, 0, 1, 2, 3, 3], size=groups)
        info[:, 1] = rng.integers(0, 5, size=groups)   # k
        info[:, 4] = rng.integers(0, 6, size=groups)   # n_orig
        infos.append(info)
    grp = dict(pkt_first=np.concatenate([[0], np.cumsum(new_counts)]).astype(np.int32), pkt_off=rec_off[n_prev:].copy(),
               pkt_len=rec_len[n_prev:].copy(), pkt_dg=rng.permutation(n_new).astype(np.int32),
               slot_group=(s32(P + shift) + np.arange(groups)).astype(np.int32))
    hold = int(np.sum((rec_len[:n_prev].astype(np.int64) + ALIGN - 1) // ALIGN * ALIGN)) + ALIGN
    return dict(groups=groups, prev=prev, infos=infos, grp=grp, datagrams=n_new, src=src, hold_mis=hold_mis,
                capacity=n_prev + n_new + 2, hold_bytes=hold)


# ---------------------------------------------------------------- GPU: movement, scan, slots, lengths

@pytest.mark.gpu
def test_window_movement(sh):
    """A fresh receiver; the window moving by 0, 1, groups - 1, groups and groups + 5; the group call's window
    behind the previous one; across the 32-bit wrap; 0, 1 and 4 listings with every status and done code."""
    rng = np.random.default_rng(1)
    G = 21
    seen = collections.Counter()
    for P in (1000, 2**31 - 4, -3):
        for shift in (0, 1, G - 1, G, G + 5, -1, -3, -G, -G - 2):
            for n_info in ((0, 1, 4) if P == 1000 else (2,)):
                c = make_case(rng, G, shift=shift, n_info=n_info, P=P, hold_mis=int(rng.integers(0, 16)))
                want = check(sh, c, (P, shift, n_info), variants=(0,) if P != 1000 else (0, 1))
                assert int(want["base"][0]) == s32(P + max(shift, 0))
                seen.update(int(v) for v in want["done"])
                for j, key in enumerate(("carried", "newly", "expired", "ignored", "below")):
                    seen[key] += int(want["summary"][(1, 3, 4, 5, 6)[j]])
                if n_info == 0:
                    assert want["summary"][3] == 0
                if shift >= G:
                    assert want["summary"][1] == 0 and want["summary"][5] == 0 and not want["done"].any()
                if shift <= -G:
                    assert want["summary"][0] == want["summary"][1] and want["summary"][6] == c["datagrams"]
    assert all(seen[key] > 0 for key in (0, 1, 2, 3, "carried", "newly", "expired", "ignored", "below"))
    c = make_case(rng, G, shift=2)
    want = want_of(c, c["hold_bytes"], fresh=True)
    assert want["base"][0] == 1002 and want["summary"][0] == c["datagrams"] and not want["summary"][1:].any()


@pytest.mark.gpu
@pytest.mark.parametrize("groups", [1, 2, 15, 16, 17, SCAN_PASS - 1, SCAN_PASS, SCAN_PASS + 1, 2 * SCAN_PASS + 1])
def test_window_scan_boundaries(sh, groups):
    rng = np.random.default_rng(groups)
    for shift in (0, 3):
        c = make_case(rng, groups, shift=shift, n_info=1, prev_counts=rng.integers(0, 3, size=groups),
                      new_counts=rng.integers(0, 3, size=groups), lens=(2, 9, 16, 33))
        want = check(sh, c, (groups, shift), variants=(0,))
        assert want["first"][-1] == want["summary"][0]
        assert groups < 15 or shift or (want["summary"][1] > 0 and want["summary"][0] > groups // 4)


@pytest.mark.gpu
def test_window_records_per_slot(sh):
    """Slots of 0, 1, 511, 512 and 513 carried and new records."""
    rng = np.random.default_rng(2)
    counts = [0, 1, 511, 512, 513, 2]
    c = make_case(rng, 6, prev_counts=counts, new_counts=counts[::-1], lens=(2, 5, 8, 21), n_info=0)
    c["prev"]["done"][:] = 0
    want = check(sh, c, "per slot")
    assert list(np.diff(want["first"])) == [a + b for a, b in zip(counts, counts[::-1])] and want["summary"][1] == sum(counts)


@pytest.mark.gpu
def test_window_lengths_at_every_alignment(sh):
    """Lengths 2, 3, 7, 8, 9, 15, 16, 17 and B + 3 at all 16 source alignments, into hold regions at all 16
    alignments; one short record ends with the ring."""
    rng = np.random.default_rng(3)
    n = len(LENS) * 16
    for hold_mis in range(16):
        c = make_case(rng, 4, prev_counts=[n - 40, 0, 25, 15], new_counts=[1, 2, 0, 3], n_info=0, hold_mis=hold_mis,
                      aligned_sources=True)
        c["prev"]["done"][:] = 0
        assert {(int(o) % 16, int(l)) for o, l in zip(c["prev"]["off"][:n], c["prev"]["len"][:n])} == \
            {(a, l) for a in range(16) for l in LENS}
        ring, hold_off = ring_of(c, c["hold_bytes"])
        assert hold_off % 16 == hold_mis
        for ln in (3, 8):  # a record that ends with the ring's last byte: the window is pulled back
            p = int(np.flatnonzero(c["prev"]["len"][:n] == ln)[hold_mis])
            c["prev"]["off"][p] = len(ring) - ln
        want = check(sh, c, hold_mis, variants=(hold_mis % 2,))
        assert want["summary"][1] == n and want["errors"] == 0


# ---------------------------------------------------------------- GPU: overflow and malformed input

@pytest.mark.gpu
def test_window_overflow(sh):
    """capacity and hold_bytes exactly sufficient and one short: the emptied suffix and the error count.
    hold_bytes == 0 copies nothing."""
    rng = np.random.default_rng(4)
    G = 40
    c = make_case(rng, G, shift=1, n_info=1)
    full = want_of(c, c["hold_bytes"])
    records, used = int(full["summary"][0]), int(full["summary"][2])
    assert records > 30 and used > 300 and full["errors"] == 0
    want = check(sh, c, "exact", hold_bytes=used, capacity=records)
    assert want["errors"] == 0 and np.array_equal(want["first"], full["first"])
    want = check(sh, c, "a record short", hold_bytes=used, capacity=records - 1)
    last = int(np.flatnonzero(np.diff(full["first"]))[-1])
    assert want["errors"] == 1 and want["done"][last] == 3 and want["summary"][7] == 1
    want = check(sh, c, "half the records", hold_bytes=used, capacity=records // 2)
    cut = int(np.flatnonzero(full["first"][1:] > records // 2)[0])
    emptied = np.flatnonzero(np.diff(full["first"])[cut:]) + cut
    assert want["errors"] == len(emptied) > 3 and (want["done"][emptied] == 3).all()
    assert (want["first"][cut:] == full["first"][cut]).all() and np.array_equal(want["done"][:cut], full["done"][:cut])
    want = check(sh, c, "a byte short", hold_bytes=used - 1)
    carrying = np.flatnonzero([int(full["first"][s + 1]) > int(full["first"][s]) and (full["dg"][full["first"][s]] == -1)
                               for s in range(G)])
    cut = int(carrying[-1])
    assert want["errors"] >= 1 and want["done"][cut] == 3 and np.array_equal(want["done"][:cut], full["done"][:cut])
    want = check(sh, c, "half the bytes", hold_bytes=used // 2)
    assert want["errors"] > 2 and want["summary"][2] <= used // 2
    want = check(sh, c, "no hold region", hold_bytes=0)
    ring, _ = ring_of(c, 0)
    assert np.array_equal(want["ring"], ring) and want["summary"][2] == 0 and want["summary"][1] == full["summary"][1]
    assert np.array_equal(want["len"], full["len"]) and want["errors"] == 0
    c["capacity"] = 0
    want = check(sh, c, "no capacity")
    assert want["errors"] == np.count_nonzero(np.diff(full["first"])) and not want["first"].any()


@pytest.mark.gpu
def test_window_malformed_input(sh):
    """Malformed spans on either side and carried records outside the ring: the slot is malformed, its
    neighbours are not, and nothing out of bounds is read."""
    rng = np.random.default_rng(5)
    G = 12
    base = make_case(rng, G, shift=0, n_info=0, prev_counts=[3] * G, new_counts=[2] * G)
    base["prev"]["done"][:] = 0
    ring, _ = ring_of(base, base["hold_bytes"])

    def variant(edits):
        c = dict(base, prev={k: np.array(v) if isinstance(v, np.ndarray) else v for k, v in base["prev"].items()},
                 grp={k: np.array(v) for k, v in base["grp"].items()})
        for (side, name, index), value in edits.items():
            c[side][name][index] = value
        return c

    huge = 2**31 - 1
    cases = [
        ("record offset -1", {("prev", "off", 4): -1}, [1]),
        ("record length -1", {("prev", "len", 7): -1}, [2]),
        ("record a byte past the ring", {("prev", "off", 10): len(ring) - int(base["prev"]["len"][10]) + 1}, [3]),
        ("record far past the ring", {("prev", "off", 13): 2**62, ("prev", "len", 14): huge}, [4]),
        ("record at the ring's end", {("prev", "off", 16): len(ring) - int(base["prev"]["len"][16])}, []),
        ("old span starts below 0", {("prev", "first", 0): -5}, [0]),
        ("old span runs backwards", {("prev", "first", 6): 3 * 6 - 4}, [5]),
        ("old span past the capacity", {("prev", "first", G): base["prev"]["capacity"] + 1}, [G - 1]),
        ("old span far away", {("prev", "first", 3): huge, ("prev", "first", 4): -huge - 1}, [2, 3, 4]),
        ("new span starts below 0", {("grp", "pkt_first", 0): -1}, [0]),
        ("new span runs backwards", {("grp", "pkt_first", 5): 2 * 5 - 3}, [4]),
        ("new span past the datagrams", {("grp", "pkt_first", G): 2 * G + 1}, [G - 1]),
        ("both sides", {("grp", "pkt_first", 8): huge, ("prev", "first", 8): huge}, [7, 8]),
        ("a done slot's new span is not looked at", {("grp", "pkt_first", 0): -1, ("prev", "done", 0): 1}, []),
    ]
    for tag, edits, bad in cases:
        c = variant(edits)
        want = check(sh, c, tag, variants=(0,))
        assert sorted(np.flatnonzero(want["done"] == 2)) == bad, tag
        assert want["errors"] == len(bad) == want["summary"][7], tag
        assert all(want["first"][s + 1] == want["first"][s] for s in bad), tag
        assert want["summary"][0] >= 5 * (G - len(bad) - 1), tag  # the neighbours keep their records


# ---------------------------------------------------------------- GPU: a streaming receiver on the device

def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev_bucket_lazy(sh, ring, cap, G, win, kmin, kmax, m, B, decode=True):
    """list -> frame -> decode -> unframe over a window for one (k range, m, B) bucket with upper bounds (route
    (b) of INTEGRATION 2f). Every result stays on the device: nothing is read on the host here."""
    import torch
    i32 = lambda k: torch.full((k,), -9, dtype=torch.int32, device="cuda")  # noqa: E731
    u8 = lambda k: torch.full((k,), 0x77, dtype=torch.uint8, device="cuda")  # noqa: E731
    lcap = sh.rx_list_capacity(G, cap, kmax)
    r = dict(info=i32(G * INFO).view(G, INFO), lfirst=i32(G + 1), lslot=i32(G), lsum=i32(8), emax=min(kmax, m))
    loff, llen, lraw, lrows = torch.zeros(lcap, dtype=torch.int64, device="cuda"), i32(lcap), u8(lcap), u8(lcap)
    assert sh.rx_list_batch(kmin, kmax, m, B, G, cap, win.first, win.off, win.len, ring, ring.numel(), r["info"],
                            r["lfirst"], r["lslot"], loff, llen, lraw, lrows, r["lsum"],
                            u8(sh.rx_list_scratch_bytes(G, cap))) == 0
    if not decode:
        return r
    blocks = torch.zeros((lcap, B), dtype=torch.uint8, device="cuda")
    assert sh.frame_batch(B, lcap, ring, ring.numel(), loff, llen, lraw, blocks) == 0
    emax = r["emax"]
    out, out_rows, count = u8(G * emax * B).view(G, emax, B), u8(G * emax).view(G, emax), i32(G)
    assert sh.decode_batch_out_var(kmax, m, B, G, r["lfirst"], lcap, blocks, lrows, out, out_rows, count) == 0
    slots = G * emax
    pcap = slots * (B - 2)
    pay, doff, dlen = u8(pcap), torch.zeros(slots + 1, dtype=torch.int64, device="cuda"), i32(slots)
    assert sh.unframe_batch(B, G, emax, emax, out, count, pay, pcap, doff, dlen,
                            u8(sh.unframe_scratch_bytes(G, emax))) == 0
    r.update(pay=pay, doff=doff, dlen=dlen, out_rows=out_rows)
    return r


def recovered_of(r):
    """{window slot: [(id, payload)]} of a dev_bucket_lazy result, read on the host."""
    n_listed, emax = int(r["lsum"].cpu()[0]), r["emax"]
    ls, pay, doff, dlen, rows = (r[name].cpu().numpy() for name in ("lslot", "pay", "doff", "dlen", "out_rows"))
    return n_listed, {int(ls[q]): [(int(rows[q, i]), pay[doff[t]:doff[t] + dlen[t]].tobytes())
                                   for i in range(emax) for t in [q * emax + i] if dlen[t] >= 0] for q in range(n_listed)}


def device_receiver(sh, dgs, size, G, back, state0, capacity, bucket=None):
    """The datagrams `dgs` in batches of `size` through group -> window -> list -> frame -> decode -> unframe
    on the device. One allocation holds two ring regions, into which the batches are uploaded alternately,
    and two hold regions. Once batch i's window call has run, batch i - 1's ring region and hold region are
    overwritten with 0xEE: a carried payload survives only through the hold copy. With bucket = (kmax, m, B)
    there is one listing per batch and the host reads nothing until the last batch has run; without, one
    listing per (m, B) bucket that a probing listing's d_info reports, read per batch.
    Returns (per unwrapped group the delivered [(id, payload)], the sum of the window summaries)."""
    import torch
    n_all = len(dgs)
    lens = np.array([len(d) for d in dgs], np.int64)
    starts = np.concatenate([[0], np.cumsum(lens)])
    bounds = list(range(0, n_all, size)) + [n_all]
    batches = list(zip(bounds[:-1], bounds[1:]))
    region = (max(int(starts[b] - starts[a]) for a, b in batches) + 15) // 16 * 16 + 16
    hold_bytes = capacity * ((int(lens.max()) + ALIGN - 1) // ALIGN * ALIGN)
    R = [16, 16 + region]
    H = [16 + 2 * region + 5, 16 + 2 * region + 5 + hold_bytes + 11]
    total = H[1] + hold_bytes + 16
    alloc = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
    staging = _dev(np.frombuffer(b"".join(dgs), np.uint8).copy())
    all_off = np.zeros(n_all, np.int64)
    for i, (a, b) in enumerate(batches):
        all_off[a:b] = starts[a:b] - starts[a] + R[i & 1]
    d_off, d_len, state = _dev(all_off), _dev(lens.astype(np.int32)), _dev(np.array([state0], np.int32))
    W = [sh.RxWindow(G, capacity), sh.RxWindow(G, capacity)]
    scratch = torch.zeros(sh.rx_window_scratch_bytes(G, capacity), dtype=torch.uint8, device="cuda")
    kept, infos = [], []
    sh.batch_errors()
    for i, (a, b) in enumerate(batches):
        alloc[R[i & 1]:R[i & 1] + int(starts[b] - starts[a])] = staging[int(starts[a]):int(starts[b])]
        grp = dev_group(sh, alloc, d_off[a:b], d_len[a:b], state, state, G, back)
        nxt, prev = W[i & 1], W[(i - 1) & 1] if i else None
        summ = torch.zeros(8, dtype=torch.int64, device="cuda")
        assert sh.rx_window_batch(G, prev, infos, b - a, grp["pkt_first"], grp["pkt_off"], grp["pkt_len"], grp["pkt_dg"],
                                  grp["slot_group"], alloc, total, H[i & 1], hold_bytes, nxt, summ, scratch) == 0
        if i:  # the regions of the batch before are free again
            q = (i - 1) & 1
            alloc[R[q]:R[q] + region] = 0xEE
            alloc[H[q]:H[q] + hold_bytes] = 0xEE
        if bucket is None:
            probe = dev_bucket_lazy(sh, alloc, capacity, G, nxt, 2, 255, 1, 8, decode=False)
            info = probe["info"].cpu().numpy()
            found = sorted({(int(m), int(B)) for st, _, m, B in info[:, :4] if st in (1, 3)})
            assert len(found) <= MAX_INFO
            runs = [dev_bucket_lazy(sh, alloc, capacity, G, nxt, 2, 256 - m, m, B) for m, B in found]
            infos = [r["info"] for r in runs] or [probe["info"]]
            k1 = probe["info"]
        else:
            kmax, m, B = bucket
            runs = [dev_bucket_lazy(sh, alloc, capacity, G, nxt, 2, kmax, m, B)]
            infos = [runs[0]["info"]]
            k1 = runs[0]["info"]
        kept.append(dict(win={name: getattr(nxt, name).clone() for name in WIN_NAMES}, ring=alloc.clone(), summ=summ,
                         runs=runs, k1=k1))
    # only now the host looks
    errors = sh.batch_errors()
    got, sums, expect, decoded = collections.defaultdict(list), np.zeros(8, np.int64), 0, set()
    for k in kept:
        ring_h = k["ring"].cpu().numpy()
        win = {name: t.cpu().numpy() for name, t in k["win"].items()}
        base = int(win["base"][0])
        for s, recs in enumerate(records_of(win, ring_h)):  # the originals of this batch, as OnData delivers them
            got[base + s] += [(r[0], r[2:]) for r, dg in recs if dg >= 0 and r[0] <= r[1]]
        info = k["k1"].cpu().numpy()
        for s in np.flatnonzero(info[:, 0] == 2):  # the k == 1 form
            p = int(info[s, 7])
            got[base + int(s)].append((0, ring_h[win["off"][p] + 2:win["off"][p] + win["len"][p]].tobytes()))
        for r in k["runs"]:
            n_listed, rec = recovered_of(r)
            expect += G - n_listed  # the empty tail slots of route (b)
            for slot, pays in rec.items():
                assert base + slot not in decoded, "a group was decoded twice"
                decoded.add(base + slot)
                got[base + slot] += pays
        sums += k["summ"].cpu().numpy()
    assert errors == expect + int(sums[7])
    return got, sums


@pytest.mark.gpu
def test_window_streaming_chain_on_the_fixture(sh):
    """The reference client's datagrams in batches of 97: the originals, the k = 1 forms and the recovered
    payloads together are the multiset the reference's OnPacket delivered."""
    ring, dg_off, dg_len, want, _ = fixture()
    dgs = [ring[o:o + l].tobytes() for o, l in zip(dg_off, dg_len)]
    got, sums = device_receiver(sh, dgs, 97, FIX_G, FIX_BACK, 0, 1024)
    assert multiset(got) == want
    assert (sums[1], sums[5], sums[3]) == (775, 678, 13) and not sums[4] and not sums[6] and not sums[7]
    assert sums[2] > 775 * ALIGN


STREAM = [(28, 4, 136, "fixed"), (30, 6, 136, "tile"), (20, 4, 24, "generic")]


def stream_traffic(kmax, m, B):
    ora = po.oracle()
    rng = np.random.default_rng(kmax + m)
    first_group = 246  # the groups run across 255 -> 0
    ks = [int(v) for v in rng.integers(kmax - 11, kmax + 1, size=24)]
    dgs, _, arrived = interleaved_groups(rng, ora, ks, m, B, first_group)
    want = {first_group + j: sorted(orig + (opk.rx_group(ora, orig, rec) or [])) for j, (orig, rec) in enumerate(arrived)}
    return dgs, first_group, want


@pytest.mark.parametrize("shape", STREAM, ids=lambda s: "k%d_m%d_B%d_%s" % s)
def test_stream_traffic_on_the_models(shape):
    """The traffic of the device test below through the restated rules, cut the same way into the same window:
    every group delivers what the packet oracle delivers."""
    kmax, m, B, _ = shape
    dgs, first_group, want = stream_traffic(kmax, m, B)
    ring = np.frombuffer(b"".join(dgs), np.uint8)
    dg_len = np.array([len(d) for d in dgs], np.int32)
    dg_off = np.concatenate([[0], np.cumsum(dg_len)[:-1]]).astype(np.int64)
    got, sums, peak = model_receiver(dg_off, dg_len, ring, batches_of(len(dgs), 61), 12, 4, state=first_group, hold=True)
    assert {g: sorted(v) for g, v in got.items() if v} == {g: v for g, v in want.items() if v}
    assert sums[1] > 0 and sums[3] > 0 and sums[4] > 0 and peak < 512


@pytest.mark.gpu
@pytest.mark.parametrize("shape", STREAM, ids=lambda s: "k%d_m%d_B%d_%s" % s)
def test_window_streaming_chain_on_synthetic_traffic(sh, shape):
    """24 interleaved groups with loss in batches of 61 datagrams through a window of 12 slots, on a fixed, a
    tile and a generic shape: every group delivers what the packet oracle delivers, groups that lost too much
    expire, and the host reads nothing between the batches."""
    kmax, m, B, route = shape
    assert sh.path(kmax, m, B) == route
    dgs, first_group, want = stream_traffic(kmax, m, B)
    got, sums = device_receiver(sh, dgs, 61, 12, 4, first_group, 512, bucket=(kmax, m, B))
    assert {g: sorted(v) for g, v in got.items() if v} == {g: v for g, v in want.items() if v}
    assert sums[1] > 0 and sums[3] > 0 and sums[4] > 0 and not sums[7]


# ---------------------------------------------------------------- GPU: the binding on tensors, in a graph

@pytest.mark.gpu
def test_window_python_binding_graph_and_aliasing(sh):
    """group + window for two consecutive batches (A -> B, then B -> A) captured into one graph, with
    d_state_out on top of d_state_in. Between the replays the host rewrites the datagrams and the listings'
    d_info; window A carries over from one replay to the next. Every replay gives the rule's windows."""
    import torch
    from tests.test_rx_group import traffic
    rng = np.random.default_rng(70)
    n, G, back = 150, 24, 3
    region, cap = 32 * n, 4 * n
    hold_bytes = 32 * cap
    R1, R2 = 0, region
    HB, HA = 2 * region + 7, 2 * region + 7 + hold_bytes + 9
    total = HA + hold_bytes + 3
    i32 = lambda k: torch.full((k,), -9, dtype=torch.int32, device="cuda")  # noqa: E731
    s = torch.cuda.Stream()
    alloc = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
    stage2 = torch.zeros(region, dtype=torch.uint8, device="cuda")
    d_in = [dict(off=torch.zeros(n, dtype=torch.int64, device="cuda"), len=i32(n)) for _ in range(2)]
    d_grp = [dict(dg_class=i32(n), dg_slot=i32(n), pkt_first=i32(G + 1), pkt_off=torch.zeros(n, dtype=torch.int64, device="cuda"),
                  pkt_len=i32(n), pkt_dg=i32(n), slot_group=i32(G), other=i32(n), summary=i32(8),
                  scratch=torch.zeros(sh.rx_group_scratch_bytes(n, G), dtype=torch.uint8, device="cuda")) for _ in range(2)]
    d_info = [i32(G * INFO).view(G, INFO) for _ in range(2)]  # the listings over A and over B
    d_state = _dev(np.array([500], np.int32))
    WA, WB = sh.RxWindow(G, cap), sh.RxWindow(G, cap)
    d_summ = [torch.zeros(8, dtype=torch.int64, device="cuda") for _ in range(2)]
    wscratch = torch.zeros(sh.rx_window_scratch_bytes(G, cap), dtype=torch.uint8, device="cuda")

    def group(j):
        g = d_grp[j]
        assert sh.rx_group_batch(n, G, back, d_in[j]["off"], d_in[j]["len"], alloc, total, d_state, d_state, g["dg_class"],
                                 g["dg_slot"], g["pkt_first"], g["pkt_off"], g["pkt_len"], g["pkt_dg"], g["slot_group"],
                                 g["other"], g["summary"], g["scratch"]) == 0

    def window(j, prev, infos, hold_off, nxt):
        g = d_grp[j]
        assert sh.rx_window_batch(G, prev, infos, n, g["pkt_first"], g["pkt_off"], g["pkt_len"], g["pkt_dg"],
                                  g["slot_group"], alloc, total, hold_off, hold_bytes, nxt, d_summ[j], wscratch) == 0

    def run():
        group(0)
        window(0, WA, [d_info[0]], HB, WB)
        alloc[R2:R2 + region].copy_(stage2)  # batch 2 arrives once A's records in this region have been carried
        group(1)
        window(1, WB, [d_info[1]], HA, WA)

    def batch(state, at):
        """n datagrams that continue from `state`, back to back in a region at `at`: (bytes, off, len)."""
        dgs = traffic(rng, n, state)
        lens = np.array([len(d) for d in dgs], np.int32)
        assert int(lens.sum()) <= region
        data = np.full(region, FILL, np.uint8)
        data[:int(lens.sum())] = np.frombuffer(b"".join(dgs), np.uint8)
        return data, at + np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64), lens

    def random_info():
        info = rng.integers(-3, 9, size=(G, INFO)).astype(np.int32)
        info[:, 0] = rng.choice([-1, 0, 0, 0, 0, 0, 1, 1, 2, 3], size=G)
        info[:, 1], info[:, 4] = rng.integers(0, 5, size=G), rng.integers(0, 6, size=G)
        return info

    # model state: the ring, window A and the group state
    ring = np.full(total, FILL, np.uint8)
    data, off, lens = batch(500, R2)
    ring[R2:R2 + region] = data
    grp = rx_group_rule(off, lens, ring, total, 500, G, back)
    A = rx_window_rule(G, None, [], grp, n, ring, total, HA, hold_bytes, cap)
    state, errors = int(grp["state_out"][0]), int(grp["summary"][4]) + A["errors"]
    sh.batch_errors()
    with torch.cuda.stream(s):  # a fresh receiver's first batch, eagerly
        alloc[R2:R2 + region] = _dev(data)
        d_in[1]["off"].copy_(_dev(off))
        d_in[1]["len"].copy_(_dev(lens))
        group(1)
        window(1, None, [], HA, WA)
    s.synchronize()

    def compare(win, want, tag):
        for name in WIN_NAMES:
            got = getattr(win, name).cpu().numpy()
            bad = np.flatnonzero(got != want[name])
            assert not len(bad), (tag, name, bad[:6], got[bad[:6]], want[name][bad[:6]])

    compare(WA, A, "fresh")
    graph = None
    for rnd in range(3):  # eagerly once (this loads every kernel before the capture), then two replays
        data1, off1, len1 = batch(state, R1)
        ring[R1:R1 + region] = data1
        grp1 = rx_group_rule(off1, len1, ring, total, state, G, back)
        info_a, info_b = random_info(), random_info()
        B = rx_window_rule(G, A, [info_a], grp1, n, ring, total, HB, hold_bytes, cap)
        ring = np.array(B["ring"])
        data2, off2, len2 = batch(int(grp1["state_out"][0]), R2)
        ring[R2:R2 + region] = data2
        grp2 = rx_group_rule(off2, len2, ring, total, int(grp1["state_out"][0]), G, back)
        A = rx_window_rule(G, B, [info_b], grp2, n, ring, total, HA, hold_bytes, cap)
        ring = np.array(A["ring"])
        state = int(grp2["state_out"][0])
        errors += int(grp1["summary"][4]) + int(grp2["summary"][4]) + B["errors"] + A["errors"]
        with torch.cuda.stream(s):
            alloc[R1:R1 + region] = _dev(data1)
            stage2.copy_(_dev(data2))
            for j, (o, l) in enumerate(((off1, len1), (off2, len2))):
                d_in[j]["off"].copy_(_dev(o))
                d_in[j]["len"].copy_(_dev(l))
            d_info[0].copy_(_dev(info_a))
            d_info[1].copy_(_dev(info_b))
            for t in d_summ:
                t.fill_(-1)
            if rnd == 0:
                run()
        s.synchronize()
        if rnd == 1:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=s):
                run()
        if rnd:
            graph.replay()
            torch.cuda.synchronize()
        compare(WB, B, (rnd, "B"))
        compare(WA, A, (rnd, "A"))
        assert np.array_equal(d_summ[0].cpu().numpy(), B["summary"]) and np.array_equal(d_summ[1].cpu().numpy(), A["summary"])
        assert np.array_equal(alloc.cpu().numpy(), ring), rnd
        assert int(d_state.cpu()[0]) == state
        assert B["summary"][1] > 0 and A["summary"][1] > 0 and B["summary"][5] > 0
    assert sh.batch_errors(s.cuda_stream) == errors
