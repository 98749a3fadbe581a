"""znippy_unxz_batch on generated xz files: the call and its stages against Python's lzma (liblzma) on one thread and on a pool of 16
(files are independent and the GIL is released while liblzma runs; one file is one thread's work either way).
Rounds are interleaved A, A': the two series of the call give its own spread (A/A), which is the margin of every ratio beside it.
Figures are medians of the wall clock of the call, the device idle in front; stage times are the kernel times of the last call.
A block is one wave's work, so "per wave" is the decode stage's time over the bytes of the largest block.
  1. 1,400 files of 1-8 KiB
  2. 200 files of 1 MiB of content
  3. one text file of 64 MiB of content as 1 block, as blocks of 24 MiB and as blocks of 1 MiB
  4. one incompressible file (uncompressed chunks)
The tool measures and promises nothing; the tests assert none of it.

Usage: python tools/unxz_report.py [--rounds 5] [--big 64] [--preset 1] [--out profiles/unxz_report.log]"""
import argparse
import lzma
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
ap.add_argument("--preset", type=int, default=1, help="xz preset of the generated files (the dictionary is 8 MiB whatever it is)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unxz_report.log"))
args = ap.parse_args()
log = open(args.out, "w")


def say(line=""):
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()


import torch, gen, xz_build as X  # noqa: E402
from znippy_amd import hip  # noqa: E402

med = statistics.median
STAGES = ("tail", "decode", "check")


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
            st, ol, _, blocks, _ = self.ctx.unxz_sizes(self.d_src, self.off, self.len)
        else:
            st, _, ol, _, blocks, _ = self.ctx.unxz_batch(self.d_src, self.off, self.len, self.d_out, self.rooms)
        dt = time.perf_counter() - t
        assert not st.any() and [int(x) for x in ol] == self.rooms, st[:8]
        self.blocks = int(blocks.sum())
        self.kt = {s: 0.0 for s in STAGES}
        self.rounds = 0
        for k, v in self.ctx.kernel_times():
            self.kt[k[5:]] += v
            self.rounds += k == "unxz_tail"
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


def liblzma(files, threads, repeats=2):
    best = 1e9
    with ThreadPoolExecutor(threads) as ex:
        for _ in range(repeats):
            t = time.perf_counter()
            n = sum(len(x) for x in (ex.map(lzma.decompress, files) if threads > 1 else map(lzma.decompress, files)))
            best = min(best, time.perf_counter() - t)
    return best * 1e3, n


def report(name, b, rounds, pool=True, largest=None):
    """largest: (compressed, content) bytes of the largest block, the wave the decode stage waits for"""
    total = sum(b.rooms)
    a, a2 = b.measure(rounds)
    lo, hi = min(a, a2), max(a, a2)
    say(f" {name}: {len(b.files)} files, {sum(b.len)} source bytes -> {total} content bytes, {b.blocks} blocks, {b.rounds} tail round(s)")
    say(f"   unxz_batch {lo:.2f} / {hi:.2f} ms (two series: A/A spread {100 * (hi - lo) / lo:.1f} %), {total / lo / 1e6:.3f} GB/s | stages ms: {b.stages()}")
    dominant = max(STAGES, key=lambda s: b.kt[s])
    say(f"   the stage that dominates: {dominant} ({100 * b.kt[dominant] / sum(b.kt.values()):.0f} % of the stage time)")
    if largest:
        say(f"   decode: {b.kt['decode']:.2f} ms; the largest block has {largest[0]} compressed and {largest[1]} content bytes -> "
            f"{largest[0] / b.kt['decode'] / 1e3:.3f} MB/s compressed, {largest[1] / b.kt['decode'] / 1e3:.3f} MB/s content per wave")
    m, m2 = b.measure(max(2, rounds // 2), sizes=True)
    say(f"   measure mode {min(m, m2):.2f} / {max(m, m2):.2f} ms | stages ms: {b.stages()}")
    z1, n1 = liblzma(b.files, 1)
    assert n1 == total
    line = f"   liblzma (lzma.decompress): 1 thread {z1:.1f} ms -> liblzma / call = {z1 / hi:.3f} .. {z1 / lo:.3f}"
    if pool:
        z16, _ = liblzma(b.files, 16)
        line += f"; 16 threads {z16:.1f} ms -> {z16 / hi:.3f} .. {z16 / lo:.3f}"
    else:
        line += "; 16 threads: the same, one file is one thread's work"
    say(line)
    say()


def largest_block(files_blocks):
    return max(((len(b.raw), b.uncomp) for b in files_blocks), key=lambda x: x[1])


ctx = hip.Context(0)
pool = ThreadPoolExecutor(16)
say(f"device {torch.cuda.get_device_name(0)}  rounds {args.rounds}  xz preset {args.preset}, dictionary 8 MiB, CRC32 checks")
say("1. small files")
base = gen.pseudo_text(2 << 20, seed=77)
contents = []
for i in range(1400):
    size = 2500 + (i * 7919) % 24_000                           # about 1-8 KiB of xz
    at = (i * 65537) % (len(base) - size)
    contents.append(base[at:at + size])
made = list(pool.map(lambda c: X.Block(c, X.CHECK_CRC32, preset=args.preset, dict_size=8 << 20), contents))
files = [X.stream([b], X.CHECK_CRC32) for b in made]
say(f"   ({min(map(len, files))}-{max(map(len, files))} source bytes each)")
report("1,400 files of 1-8 KiB", Batch(ctx, files, contents), args.rounds, largest=largest_block(made))
say("2. files of 1 MiB of content")
contents = [text(1 << 20, seed=1000 + 3 * k) for k in range(200)]
made = list(pool.map(lambda c: X.Block(c, X.CHECK_CRC32, preset=args.preset, dict_size=8 << 20), contents))
report("200 files of 1 MiB", Batch(ctx, [X.stream([b], X.CHECK_CRC32) for b in made], contents), max(2, args.rounds // 2), largest=largest_block(made))
say(f"3. one text file of {args.big} MiB of content (gen.pseudo_text)")
cb = text(args.big << 20)
for name, block in ((f"{args.big} MiB as blocks of 1 MiB", 1 << 20), (f"{args.big} MiB as blocks of 24 MiB", 24 << 20), (f"{args.big} MiB as 1 block", len(cb))):
    parts = [cb[i:i + block] for i in range(0, len(cb), block)]
    made = list(pool.map(lambda p: X.Block(p, X.CHECK_CRC32, preset=args.preset, dict_size=8 << 20), parts))
    report(name, Batch(ctx, [X.stream(made, X.CHECK_CRC32)], [cb]), 1 if block >= (8 << 20) else max(2, args.rounds // 2), pool=False, largest=largest_block(made))
del cb
say("4. one incompressible file of 16 MiB as blocks of 1 MiB (uncompressed chunks: the wave copies)")
c = np.random.default_rng(9).bytes(16 << 20)
parts = [c[i:i + (1 << 20)] for i in range(0, len(c), 1 << 20)]
made = list(pool.map(lambda p: X.Block(p, X.CHECK_CRC32, preset=args.preset, dict_size=8 << 20), parts))
assert all(k[0] in (0, 1, 2) for b in made for k in X.chunks_of(b.raw))
report("16 MiB of random bytes", Batch(ctx, [X.stream(made, X.CHECK_CRC32)], [c]), args.rounds, pool=False, largest=largest_block(made))
ctx.close()
log.close()
