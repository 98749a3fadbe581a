"""znippy_bunzip2_batch on generated bzip2 files: the call and its stages against Python's bz2 (libbz2) on one thread and on a pool
of 16 (files are independent and the GIL is released while libbz2 runs; one file is one thread's work either way).
Rounds are interleaved A, B, A': the two series of the call give its own spread (A/A), which is the margin of every ratio beside it.
Figures are medians of the wall clock of the call, the device idle in front; stage times are the kernel times of the last call,
summed over its passes.  The decode figure counts content bytes, which for text are the bytes of a block in front of the inverse BWT
and an upper bound on its symbols.
  1. one level-9 text file of 8 MiB and one of 64 MiB of content
  2. 1,400 files of 1-8 KiB
  3. 200 files of 1 MiB of content
  4. the walk stage against the same stage with one sublist per block (ZNIPPY_BZ_SPLIT above the block length), and a sweep of the spacing
The tool measures and promises nothing; the tests assert none of it.

Usage: python tools/bunzip2_report.py [--rounds 5] [--big 64] [--out profiles/bunzip2_report.log]"""
import argparse
import bz2
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--big", type=int, default=64, help="MiB of content of the big file")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bunzip2_report.log"))
args = ap.parse_args()
log = open(args.out, "w")


def say(line=""):
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()


import torch, gen  # noqa: E402
from znippy_amd import hip  # noqa: E402

med = statistics.median
STAGES = ("scan", "decode", "walk", "expand", "crc")


def text(size, seed=300):
    return b"".join(gen.pseudo_text(2 << 20, seed=seed + k) for k in range(max(1, (size + (2 << 20) - 1) >> 21)))[:size]


class Batch:
    def __init__(self, ctx, files, contents):
        self.ctx, self.files, self.contents = ctx, files, contents
        self.off = np.concatenate([[0], np.cumsum([len(f) for f in files])[:-1]]).astype(np.uint64)
        self.len = [len(f) for f in files]
        self.d_src = torch.from_numpy(np.frombuffer(b"".join(files) + bytes(64), np.uint8).copy()).cuda()
        self.rooms = [len(c) for c in contents]
        self.d_out = torch.zeros(sum(self.rooms) + 64, dtype=torch.uint8, device="cuda")

    def call(self, sizes=False):
        torch.cuda.synchronize(); self.ctx.sync()
        t = time.perf_counter()
        if sizes:
            st, ol, _, blocks = self.ctx.bunzip2_sizes(self.d_src, self.off, self.len)
        else:
            st, _, ol, _, blocks = self.ctx.bunzip2_batch(self.d_src, self.off, self.len, self.d_out, self.rooms)
        dt = time.perf_counter() - t
        assert not st.any() and [int(x) for x in ol] == self.rooms, st[:8]
        self.blocks = int(blocks.sum())
        self.kt = {s: 0.0 for s in STAGES}
        self.passes = 0
        for k, v in self.ctx.kernel_times():
            self.kt[k[8:]] += v
            self.passes += k == "bunzip2_decode"
        return dt * 1e3

    def check(self):
        assert self.d_out[:sum(self.rooms)].cpu().numpy().tobytes() == b"".join(self.contents)

    def measure(self, rounds, sizes=False):
        self.call(sizes)
        if not sizes:
            self.check()
        a, a2 = [], []
        for _ in range(rounds):
            a.append(self.call(sizes))
            a2.append(self.call(sizes))
        return med(a), med(a2)

    def stages(self):
        return ", ".join(f"{s} {self.kt[s]:.3f}" for s in STAGES if self.kt[s])


def libbz2(files, threads, repeats=2):
    best = 1e9
    with ThreadPoolExecutor(threads) as ex:
        for _ in range(repeats):
            t = time.perf_counter()
            n = sum(len(x) for x in (ex.map(bz2.decompress, files) if threads > 1 else map(bz2.decompress, files)))
            best = min(best, time.perf_counter() - t)
    return best * 1e3, n


def report(name, b, rounds, pool=True):
    total = sum(b.rooms)
    a, a2 = b.measure(rounds)
    lo, hi = min(a, a2), max(a, a2)
    say(f" {name}: {len(b.files)} files, {sum(b.len)} source bytes -> {total} content bytes, {b.blocks} blocks, {b.passes} passes")
    say(f"   bunzip2_batch {lo:.2f} / {hi:.2f} ms (two series: A/A spread {100 * (hi - lo) / lo:.1f} %), {total / lo / 1e6:.3f} GB/s | stages ms: {b.stages()}")
    dominant = max(STAGES, key=lambda s: b.kt[s])
    say(f"   the stage that dominates: {dominant} ({100 * b.kt[dominant] / sum(b.kt.values()):.0f} % of the stage time)")
    if b.blocks:
        per_block = total / b.blocks
        say(f"   decode: {b.kt['decode']:.2f} ms over {b.passes} passes of concurrent waves; a wave has {per_block:.0f} content bytes per block -> "
            f"about {per_block * b.passes / b.kt['decode'] / 1e3:.2f} M bytes (symbols at the most) per second per wave")
    m, m2 = b.measure(max(2, rounds // 2), sizes=True)
    say(f"   measure mode {min(m, m2):.2f} / {max(m, m2):.2f} ms | stages ms: {b.stages()}")
    z1, n1 = libbz2(b.files, 1)
    assert n1 == total
    line = f"   libbz2 (bz2.decompress): 1 thread {z1:.1f} ms -> libbz2 / call = {z1 / hi:.2f} .. {z1 / lo:.2f}"
    if pool:
        z16, _ = libbz2(b.files, 16)
        line += f"; 16 threads {z16:.1f} ms -> {z16 / hi:.2f} .. {z16 / lo:.2f}"
    else:
        line += "; 16 threads: the same, one file is one thread's work"
    say(line)
    say()


def with_split(value, fn):
    old = os.environ.get("ZNIPPY_BZ_SPLIT")
    if value is None:
        os.environ.pop("ZNIPPY_BZ_SPLIT", None)
    else:
        os.environ["ZNIPPY_BZ_SPLIT"] = str(value)
    try:
        return fn()
    finally:
        if old is None:
            os.environ.pop("ZNIPPY_BZ_SPLIT", None)
        else:
            os.environ["ZNIPPY_BZ_SPLIT"] = old


def walk_cases(b, rounds):
    say(f" 4. the walk stage on the {len(b.contents[0]) >> 20} MiB file ({b.blocks} blocks of 900,000 bytes, a workgroup each), ms, rounds interleaved")
    series = {"default": [], "default again": [], "one sublist": []}
    for _ in range(rounds):
        for name, split in (("default", None), ("one sublist", 4_000_000_000), ("default again", None)):
            with_split(split, b.call)
            series[name].append(b.kt["walk"])
    d, d2, one = med(series["default"]), med(series["default again"]), med(series["one sublist"])
    lo, hi = min(d, d2), max(d, d2)
    say(f"   default spacing {lo:.3f} / {hi:.3f} (A/A spread {100 * (hi - lo) / lo:.1f} %) | one sublist per block {one:.3f} -> one sublist / default = {one / hi:.2f} .. {one / lo:.2f}")
    sweep = []
    for split in (16, 32, 64, 128, 256, 512, 1024, 4096, 16384, 65536):
        t = []
        for _ in range(max(3, rounds // 2 + 1)):
            with_split(split, b.call)
            t.append(b.kt["walk"])
        sweep.append((split, med(t)))
    say("   spacing -> walk ms: " + ", ".join(f"{s}: {t:.3f}" for s, t in sweep))
    say(f"   best of the sweep: {min(sweep, key=lambda x: x[1])[0]}")
    say()


ctx = hip.Context(0)
say(f"device {torch.cuda.get_device_name(0)}  rounds {args.rounds}  ZNIPPY_BZ_SPLIT {os.environ.get('ZNIPPY_BZ_SPLIT', 'as built')}  "
    f"ZNIPPY_BZ_SCRATCH_MB {os.environ.get('ZNIPPY_BZ_SCRATCH_MB', 'as built')}")
say("1. single level-9 text files (gen.pseudo_text)")
c8 = text(8 << 20)
b8 = Batch(ctx, [bz2.compress(c8, 9)], [c8])
report("8 MiB", b8, args.rounds, pool=False)
cb = text(args.big << 20)
bb = Batch(ctx, [bz2.compress(cb, 9)], [cb])
report(f"{args.big} MiB", bb, max(2, args.rounds // 2), pool=False)
del bb, cb
say("2. small files")
base = gen.pseudo_text(2 << 20, seed=77)
contents = []
for i in range(1400):
    size = 2500 + (i * 7919) % 24_000                           # about 1-8 KiB of bzip2
    at = (i * 65537) % (len(base) - size)
    contents.append(base[at:at + size])
files = [bz2.compress(c, 9) for c in contents]
say(f"   ({min(map(len, files))}-{max(map(len, files))} source bytes each)")
report("1,400 files of 1-8 KiB", Batch(ctx, files, contents), args.rounds)
say("3. files of 1 MiB of content")
contents = [text(1 << 20, seed=1000 + 3 * k) for k in range(200)]
files = [bz2.compress(c, 9) for c in contents]
report("200 files of 1 MiB", Batch(ctx, files, contents), max(2, args.rounds // 2))
walk_cases(b8, args.rounds)
ctx.close()
log.close()
