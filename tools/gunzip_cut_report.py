"""znippy_gunzip_batch with the cut at block starts (znippy_ctx_set_gunzip_cut) on generated gzip files without flush points: what
cutting them buys over the one wave they get otherwise, stage by stage, and what the search costs where nothing is cut.
Per input: the call with the search off and on, rounds interleaved A (on), B, B (off): the two B series give the off side's own spread
(A/A), which is the margin of the ratio; the stage times (summed over the passes); the counters; zlib on one thread; the window swept
from 4 KiB to 256 KiB; and the scratch budget at 64 MB against the default.
Inputs: gen.text, gen.pseudo_text and gen.binary at each of --mib, zlib level 6, one member, no flush; pseudo_text also at levels 1 and
9 (up to 64 MiB: the one wave of the switch off takes 12.7 s per call on 64 MiB of level 1); a pigz-like file (a sync flush every
128 KiB); and the 1,400 small files of tools/gunzip_report.py.  Sizes of 512 MiB and more are measured in one round.
Figures are medians of the wall clock of the call, the device idle in front; the kernel times are those of the last call.  The tool
measures and promises nothing; the tests assert none of it.

Usage: python tools/gunzip_cut_report.py [--rounds 3] [--mib 8,64,512] [--out profiles/gunzip_cut_report.log] [--no-small]"""
import argparse
import os
import statistics
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--mib", default="8,64,512")
ap.add_argument("--no-small", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gunzip_cut_report.log"))
args = ap.parse_args()
log = open(args.out, "w")


def say(line=""):
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()


import torch, gen  # noqa: E402
from znippy_amd import hip  # noqa: E402

import re  # noqa: E402
med = statistics.median
# the value the tools turn the switch on with: include/znippy_hip.h has it
CUT = int(re.search(r"#define ZNIPPY_GZ_CUT_DEFAULT (\d+)", open(os.path.join(ROOT, "include", "znippy_hip.h")).read()).group(1))
SWEEP = tuple(k << 10 for k in (4, 8, 16, 32, 64, 128, 256))


def gz(content, level=6, flush_every=None):
    c = zlib.compressobj(level, zlib.DEFLATED, 31)
    if flush_every is None:
        return c.compress(content) + c.flush()
    out = b""
    for at in range(0, len(content), flush_every):
        out += c.compress(content[at:at + flush_every]) + c.flush(zlib.Z_SYNC_FLUSH)
    return out + c.flush()


class Batch:
    def __init__(self, ctx, files, rooms):
        self.ctx = ctx
        self.off = np.concatenate([[0], np.cumsum([len(f) for f in files])[:-1]]).astype(np.uint64)
        self.len = [len(f) for f in files]
        self.d_src = torch.from_numpy(np.frombuffer(b"".join(files) + bytes(64), np.uint8).copy()).cuda()
        self.rooms = rooms
        self.d_out = torch.zeros(sum(rooms) + 64, dtype=torch.uint8, device="cuda")

    def call(self, cut):
        self.ctx.set_gunzip_cut(cut)
        torch.cuda.synchronize(); self.ctx.sync()
        t = time.perf_counter()
        st, _, ol, _, seg = self.ctx.gunzip_batch(self.d_src, self.off, self.len, self.d_out, self.rooms)
        dt = time.perf_counter() - t
        assert not st.any() and [int(x) for x in ol] == self.rooms, st[:8]
        self.kt = {}
        for k, v in self.ctx.kernel_times():                    # (a stage runs once per pass)
            self.kt[k] = self.kt.get(k, 0.0) + v
        self.stats, self.segments = self.ctx.gunzip_cut_stats(), int(seg.sum())
        return dt * 1e3

    def measure(self, cut, rounds):
        self.call(cut)
        if rounds > 1:
            self.call(0)
        a, b1, b2 = [], [], []
        for _ in range(rounds):
            a.append(self.call(cut))
            on = (self.kt, self.stats, self.segments)
            b1.append(self.call(0))
            b2.append(self.call(0))
        return med(a), (med(b1), med(b2)), on


def report(name, ctx, files, contents, sweep=True, cut=CUT):
    src, out = sum(map(len, files)), sum(map(len, contents))
    b = Batch(ctx, files, [len(c) for c in contents])
    a, (lo, hi), (kt, stats, seg_on) = b.measure(cut, args.rounds if out < 512 << 20 else 1)
    lo, hi = min(lo, hi), max(lo, hi)
    t = time.perf_counter()
    for f in files:
        zlib.decompress(f, 31)
    z = (time.perf_counter() - t) * 1e3
    find = kt.get("gunzip_find", 0.0)
    say(f" {name}: {len(files)} file(s), {src} source bytes -> {out} content bytes, segments {b.segments} off, {seg_on} on")
    say(f"   off {lo:.3f} / {hi:.3f} ms (two series: A/A spread {100 * (hi - lo) / lo:.1f} %)   on (cut {cut}) {a:.3f} ms ({out / a / 1e6:.3f} GB/s)   off / on = {lo / a:.2f} .. {hi / a:.2f}"
        f"   zlib, one thread {z:.2f} ms")
    say(f"   find {find:.3f} ms" + (f" ({src / find / 1e6:.2f} GB/s of source, {stats[0] / find / 1e6:.1f} G positions/s)" if find else " (not launched)") +
        f"   other kernels ms: {', '.join(f'{k[7:]} {v:.3f}' for k, v in kt.items() if k != 'gunzip_find')}   on / zlib = {a / z:.2f}")
    say(f"   stats: tested {stats[0]}, passed {stats[1]}, kept {stats[2]}, landed {stats[3]}, marker pieces {stats[4]}, direct pieces {stats[5]}, markers resolved {stats[6]}, passes {stats[7]}")
    if sweep:
        parts = []
        for c in SWEEP:
            t = b.call(c)
            t = min(t, b.call(c))
            parts.append(f"cut {c >> 10} KiB: kept {b.stats[2]}, landed {b.stats[3]}, call {t:.2f} ms")
        say("   sweep (best of two calls): " + " | ".join(parts))
        os.environ["ZNIPPY_GZ_CUT_SCRATCH_MB"] = "64"
        t = min(b.call(cut), b.call(cut))
        del os.environ["ZNIPPY_GZ_CUT_SCRATCH_MB"]
        say(f"   budget 64 MB: call {t:.2f} ms, {b.stats[7]} passes (default budget: {stats[7]})")
    b.ctx.set_gunzip_cut(0)


def small_files(n=1400):
    base = gen.pseudo_text(2 << 20, seed=77)
    files, contents = [], []
    for i in range(n):
        size = 3600 + (i * 7919) % 26_000
        at = (i * 65537) % (len(base) - size)
        contents.append(base[at:at + size])
        files.append(gz(contents[-1]))
    return files, contents


ctx = hip.Context(0)
say(f"device {torch.cuda.get_device_name(0)}  rounds {args.rounds}  sizes {args.mib} MiB  ZNIPPY_GZ_CUT_DEFAULT {CUT}")
for mib in (int(x) for x in args.mib.split(",")):
    size = mib << 20
    soup = b"".join(gen.pseudo_text(2 << 20, seed=300 + k) for k in range(max(1, size >> 21)))[:size]
    say(f"{mib} MiB of content, one member, no flush")
    report("gen.pseudo_text, level 6", ctx, [gz(soup)], [soup])
    for level in (1, 9) if mib <= 64 else ():
        report(f"gen.pseudo_text, level {level}", ctx, [gz(soup, level)], [soup], sweep=False)
    t = gen.text(size)
    report("gen.text (45-byte phrase), level 6", ctx, [gz(t)], [t], sweep=False)
    r = gen.binary(size)
    report("gen.binary, level 6", ctx, [gz(r)], [r], sweep=False)
    if mib == 8:
        report("gen.pseudo_text, a sync flush every 128 KiB (pigz-like)", ctx, [gz(soup, 6, 128 << 10)], [soup], sweep=False)
if not args.no_small:
    files, contents = small_files()
    say(f"1,400 single-member files of 1-8 KiB (cut {CUT}: none is searched; cut 64 below: all are)")
    report(f"small files, cut {CUT}", ctx, files, contents, sweep=False)
    report("small files, cut 64", ctx, files, contents, sweep=False, cut=64)
ctx.close()
log.close()
