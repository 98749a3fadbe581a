"""znippy_gunzip_batch on generated gzip files: what cutting a file at flush points and members buys over the one-wave decoder, and
what the call costs where there is nothing to cut.
Every case is measured against znippy_inflate_batch of the same raw DEFLATE stream(s) with known sizes on the same build (existing
one-wave code, not the code under test), rounds interleaved A, B, B: the two B series give the baseline's own spread (A/A), which
is the margin of every ratio.  Figures are medians of the wall clock of the call, the device idle in front; the kernel times are
those of the last call.  zlib: Python's zlib on one thread and on a pool of 16 (where the file has independent pieces: members, or
the pieces between full flushes, whose offsets the tool knows because it wrote them).
  1. 8 MiB of content as one member with a full flush every 128 KiB (64 pieces); the arithmetic ceiling is pieces / 2 = 32 times the
     one-wave call (two passes, each 1 / 64 of the chain)
  2. the same content with sync flushes (all pieces dependent) and with no flush at all: one decode, plus scan and probe in the first
  3. 1,400 single-member files of 1-8 KiB (the crate-sized batch): the price of headers, trailers and the scan
  4. BGZF: 8 MiB in 64 KiB members
  5. seg_min swept on case 1 and on a pigz-like file (a sync flush every 128 KiB)
Cases 1, 2, 4 and 5 run on the 45-byte phrase of gen.text, which compresses 300 : 1 — a piece of 128 KiB is 450 bytes of source — and
on the word soup of gen.pseudo_text (3 : 1).  The tool measures and promises nothing; the tests assert none of it.

Usage: python tools/gunzip_report.py [--rounds 7] [--mib 8] [--out profiles/gunzip_report.log]"""
import argparse
import os
import statistics
import struct
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--mib", type=int, default=8)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gunzip_report.log"))
args = ap.parse_args()
log = open(args.out, "w")


def say(line=""):
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()


import torch, gen  # noqa: E402
from znippy_amd import hip  # noqa: E402

PIECE = 128 << 10
SIZE = args.mib << 20
med = statistics.median


def member(content, flush=None, every=PIECE):
    """(file, offsets of the pieces' first bytes in the file)"""
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    out, cuts = b"", [10]
    for at in range(0, len(content), every):
        out += c.compress(content[at:at + every])
        if flush is not None and at + every < len(content):
            out += c.flush(flush)
            cuts.append(len(out))
    return out + c.flush(), cuts


def bgzf(content, size=64 << 10):
    out = []
    for at in range(0, len(content), size):
        part = content[at:at + size]
        raw = zlib.compressobj(6, zlib.DEFLATED, -15)
        body = raw.compress(part) + raw.flush()
        out.append(b"\x1f\x8b\x08\x04" + bytes(4) + b"\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", (len(body) + 25) & 0xFFFF) + body +
                   struct.pack("<II", zlib.crc32(part), len(part)))
    return out


class Batch:
    """files on the device, once; the gunzip call and the one-wave call over the same bytes"""

    def __init__(self, ctx, files, contents, streams):
        self.ctx, self.contents = ctx, contents
        self.off = np.concatenate([[0], np.cumsum([len(f) for f in files])[:-1]]).astype(np.uint64)
        self.len = [len(f) for f in files]
        self.d_src = torch.from_numpy(np.frombuffer(b"".join(files) + bytes(64), np.uint8).copy()).cuda()
        self.rooms = [len(c) for c in contents]
        self.d_out = torch.zeros(sum(self.rooms) + 64, dtype=torch.uint8, device="cuda")
        # the raw streams of the one-wave call: (file, offset in it, length, content length)
        self.s_off = [int(self.off[f]) + o for f, o, _, _ in streams]
        self.s_len = [n for _, _, n, _ in streams]
        self.s_out = [u for _, _, _, u in streams]

    def gunzip(self, seg_min=0):
        torch.cuda.synchronize(); self.ctx.sync()
        t = time.perf_counter()
        st, _, ol, mem, seg = self.ctx.gunzip_batch(self.d_src, self.off, self.len, self.d_out, self.rooms, seg_min=seg_min)
        dt = time.perf_counter() - t
        assert not st.any() and [int(x) for x in ol] == self.rooms, st[:8]
        self.kt, self.segments, self.members = dict(self.ctx.kernel_times()), int(seg.sum()), int(mem.sum())
        return dt * 1e3

    def one_wave(self):
        torch.cuda.synchronize(); self.ctx.sync()
        t = time.perf_counter()
        st, _ = self.ctx.inflate_batch(self.d_src, self.s_off, self.s_len, self.d_out, self.s_out)
        dt = time.perf_counter() - t
        assert not st.any()
        return dt * 1e3

    def check(self):
        assert self.d_out[:sum(self.rooms)].cpu().numpy().tobytes() == b"".join(self.contents)

    def measure(self, seg_min=0, baseline=True):
        self.gunzip(seg_min); self.check()
        a, b1, b2 = [], [], []
        if baseline:
            self.one_wave(); self.check()
        for _ in range(args.rounds):
            a.append(self.gunzip(seg_min))
            if baseline:
                b1.append(self.one_wave())
                b2.append(self.one_wave())
        return med(a), (med(b1), med(b2)) if baseline else None

    def kernels(self):
        return ", ".join(f"{k[7:]} {v:.3f}" for k, v in self.kt.items())


def zlib_pool(pieces, threads):
    def one(p):
        return len(zlib.decompressobj(-15).decompress(p))
    best = 1e9
    with ThreadPoolExecutor(threads) as ex:
        for _ in range(3):
            t = time.perf_counter()
            n = sum(ex.map(one, pieces)) if threads > 1 else sum(one(p) for p in pieces)
            best = min(best, time.perf_counter() - t)
    return best * 1e3, n


def line(name, b, a, base, extra=""):
    mb = sum(b.rooms) / 1e6
    say(f"  {name}: gunzip_batch {a:.3f} ms ({mb / a:.2f} GB/s), {b.members} members, {b.segments} segments | kernels ms: {b.kernels()}{extra}")
    if base:
        lo, hi = min(base), max(base)
        say(f"      one-wave inflate_batch {lo:.3f} / {hi:.3f} ms (two series: A/A spread {100 * (hi - lo) / lo:.1f} %) -> one-wave / gunzip = {lo / a:.2f} .. {hi / a:.2f}")


def one_file(ctx, f, content):
    return Batch(ctx, [f], [content], [(0, 10, len(f) - 18, len(content))])


def big_cases(ctx, name, content):
    say(f"content '{name}': {len(content)} bytes")
    # 1. full flush
    f, cuts = member(content, zlib.Z_FULL_FLUSH)
    b = one_file(ctx, f, content)
    a, base = b.measure(seg_min=1)
    pieces = [f[x:y] for x, y in zip(cuts, cuts[1:] + [len(f) - 8])]
    z1, n1 = zlib_pool([f[10:-8]], 1)
    z16, n16 = zlib_pool(pieces, 16)
    assert n1 == len(content) and n16 == len(content)
    say(f" 1. full flush every {PIECE >> 10} KiB: {len(f)} source bytes, {len(cuts)} pieces (ceiling: {len(cuts) / 2:.0f} times the one-wave call)")
    line("seg_min 1", b, a, base, f" | zlib 1 thread {z1:.2f} ms, 16 threads over the pieces {z16:.2f} ms")
    full = (b, base)
    a, _ = b.measure(baseline=False)
    line("default seg_min", b, a, None)
    # 2. sync flush, no flush
    for what, mode in (("sync flush (every piece reaches back)", zlib.Z_SYNC_FLUSH), ("no flush", None)):
        f2, _ = member(content, mode)
        b2 = one_file(ctx, f2, content)
        a, base2 = b2.measure(seg_min=1)
        say(f" 2. {what}: {len(f2)} source bytes")
        line("seg_min 1", b2, a, base2)
        if mode is not None:
            sync = b2
    # 4. BGZF
    mem = bgzf(content)
    f4 = b"".join(mem) + bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
    streams, at = [], 0
    for k, m in enumerate(mem):
        streams.append((0, at + 18, len(m) - 26, min(64 << 10, len(content) - k * (64 << 10))))
        at += len(m)
    b4 = Batch(ctx, [f4], [content], streams)
    a, base4 = b4.measure()
    z1, _ = zlib_pool([m[18:-8] for m in mem], 1)
    z16, _ = zlib_pool([m[18:-8] for m in mem], 16)
    say(f" 4. BGZF, 64 KiB members: {len(f4)} source bytes (the one-wave call gets one stream per member)")
    line("default seg_min", b4, a, base4, f" | zlib 1 thread {z1:.2f} ms, 16 threads {z16:.2f} ms")
    # 5. seg_min
    say(" 5. seg_min (source bytes) on the full-flush file and on the sync-flush file (pigz-like)")
    for sm in (256, 1 << 10, 4 << 10, 16 << 10, 64 << 10):
        a1, _ = full[0].measure(seg_min=sm, baseline=False)
        s1, k1 = full[0].segments, full[0].kernels()
        a2, _ = sync.measure(seg_min=sm, baseline=False)
        say(f"  seg_min {sm:6d}: full flush {a1:.3f} ms, {s1} segments ({k1}) | sync flush {a2:.3f} ms, {sync.segments} segments ({sync.kernels()})")
    say()


def small_files(ctx, n=1400):
    base = gen.pseudo_text(2 << 20, seed=77)
    files, contents = [], []
    for i in range(n):
        size = 3600 + (i * 7919) % 26_000                       # about 1-8 KiB of gzip
        at = (i * 65537) % (len(base) - size)
        contents.append(base[at:at + size])
        c = zlib.compressobj(6, zlib.DEFLATED, 31)
        files.append(c.compress(contents[-1]) + c.flush())
    b = Batch(ctx, files, contents, [(k, 10, len(f) - 18, len(contents[k])) for k, f in enumerate(files)])
    a, base_t = b.measure()
    z1, _ = zlib_pool([f[10:-8] for f in files], 1)
    z16, _ = zlib_pool([f[10:-8] for f in files], 16)
    say(f" 3. {n} single-member files of {min(map(len, files))}-{max(map(len, files))} bytes ({sum(map(len, files))} in all -> {sum(b.rooms)} content bytes)")
    line("default seg_min", b, a, base_t, f" | zlib 1 thread {z1:.2f} ms, 16 threads {z16:.2f} ms")
    say("      (the one-wave call gets the raw streams and their sizes; the difference is the scan, the headers, the trailers and the padding)")
    say()


ctx = hip.Context(0)
say(f"device {torch.cuda.get_device_name(0)}  rounds {args.rounds}  content {args.mib} MiB  default seg_min {os.environ.get('ZNIPPY_GZ_SEG_MIN', 'as built')}")
big_cases(ctx, "gen.text (45-byte phrase)", gen.text(SIZE))
big_cases(ctx, "gen.pseudo_text (word soup)", b"".join(gen.pseudo_text(2 << 20, seed=300 + k) for k in range(max(1, SIZE >> 21)))[:SIZE])
small_files(ctx)
ctx.close()
log.close()
