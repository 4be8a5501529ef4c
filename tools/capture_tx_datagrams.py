#!/usr/bin/env python3
"""Capture the server's side of a short run of the reference's protocol layer as the fixture
tests/golden/tx_datagrams.npz: every datagram its SendData was given, before loss, in send order, every
payload handed to Send and every message handed to SendOOB.

    python tools/capture_tx_datagrams.py --reference DIR      (or REF=DIR in the environment)

Builds tools/capture_tx_datagrams.cpp in a temporary directory against the reference's unchanged
Shorthair.cpp / PacketAllocator.cpp / SiameseTools.cpp and the reference codec (cauchy_256.cpp, gf256.cpp),
with the flags INTEGRATION section 1 quotes, runs it there and keeps only the recorded data. CPU only; it
needs the reference tree and is never run where there is none. Shorthair ticks on the wall clock, so two
captures differ; the committed one is what the tests use.

The fixture: dg_bytes uint8 (the datagrams back to back), dg_len int32; pay_bytes uint8, pay_len int32 (the
payloads handed to Send, in order); oob_bytes, oob_len likewise (the messages handed to SendOOB); stats int64
[sent, delivered, oob_delivered, wire_packets, wire_dropped].
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
OUT = os.path.join(ROOT, "tests", "golden", "tx_datagrams.npz")
LIMIT = os.path.getsize(os.path.join(ROOT, "tests", "golden", "c1_capture.npz"))
MSCXX = os.environ.get("MSCXX", "/opt/rocm/lib/llvm/bin/clang++")
MSFLAGS = ["-std=c++14", "-O2", "-w", "-fms-compatibility", "-fms-compatibility-version=19", "-fgnuc-version=11.4",
           "-fno-delayed-template-parsing", "-D__STDC__=1", "-include", "cstring", "-march=x86-64-v3"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("REF"), required="REF" not in os.environ,
                    help="the reference tree (catid/shorthair), read in place")
    ap.add_argument("--seconds", default="1.3")
    ap.add_argument("--per-tick", default="4")
    ap.add_argument("--max-bytes", default="40")
    args = ap.parse_args()
    ref = args.reference
    srcs = [os.path.join(ref, f) for f in ("Shorthair.cpp", "PacketAllocator.cpp", "SiameseTools.cpp",
                                           "cauchy_256.cpp", "gf256.cpp")]
    with tempfile.TemporaryDirectory() as d:
        exe, rec = os.path.join(d, "capture_tx_datagrams"), os.path.join(d, "capture.bin")
        subprocess.run([MSCXX] + MSFLAGS + [f"-I{ref}", "-o", exe, os.path.join(ROOT, "tools", "capture_tx_datagrams.cpp")]
                       + srcs + ["-lpthread"], check=True)
        r = subprocess.run([exe, "--out", rec, "--seconds", args.seconds, "--per-tick", args.per_tick,
                            "--max-bytes", args.max_bytes], capture_output=True, text=True, timeout=120, check=True)
        stats = json.loads(r.stdout.strip().splitlines()[-1])
        print(stats)
        b = open(rec, "rb").read()
    lists = {0: [], 1: [], 2: []}
    at = 0
    while at < len(b):
        kind, n = b[at], b[at + 1] | (b[at + 2] << 8)
        lists[kind].append(b[at + 3:at + 3 + n])
        at += 3 + n
    assert at == len(b)
    arrays = {"stats": np.array([stats[k] for k in ("sent", "delivered", "oob_delivered", "wire_packets",
                                                    "wire_dropped")], np.int64)}
    for name, items in (("dg", lists[0]), ("pay", lists[1]), ("oob", lists[2])):
        arrays[name + "_bytes"] = np.frombuffer(b"".join(items), np.uint8)
        arrays[name + "_len"] = np.array([len(x) for x in items], np.int32)
    assert len(lists[0]) == stats["wire_packets"] and len(lists[1]) == stats["sent"]
    np.savez_compressed(OUT, **arrays)
    size = os.path.getsize(OUT)
    print("wrote", os.path.relpath(OUT, ROOT), size, "bytes:", len(lists[0]), "datagrams,", len(lists[1]), "payloads,",
          len(lists[2]), "out-of-band messages")
    assert size <= LIMIT, "the fixture must not be larger than c1_capture.npz"


if __name__ == "__main__":
    sys.exit(main())
