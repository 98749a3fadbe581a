"""znippy_inflate_batch against Python's zlib on 16 threads, in one process.
  poms   N entries of 1-8 KiB of the xml-like text C5's small files are made of (default N = 1,400, C5's jar count), deflated at level 6:
         the batch the ingest plugins make — one small entry per jar.  That text is periodic (a pom is a few dozen long matches), so the
         same sizes run again as non-periodic word soup
  big    a set of entries of 100 KiB - 2 MiB of non-periodic text, one batch; then each of them alone, which is one wave's time for it
Per batch: call time by the wall clock (best and median of `rounds`, the device idle in front), the `inflate` and `inflate_crc` kernel
times, and the same batch through zlib.decompressobj(-15) + zlib.crc32 on a pool of 16 threads and on one thread.  Symbols per second
per wave: the literal/length symbols of an entry (counted by a small decoder in this file, on a sample, scaled by content bytes)
over the kernel time of that entry decoded alone; last, an entry of literals only and one of longest matches only.  The tests assert
none of this.  Last, the read side's call: znippy_archive_extract_zip_entries over an archive of n_poms jars, stored and compressed, against
zipfile over the same jars as files.

Usage: python tools/inflate_report.py [n_poms=1400] [rounds=7]"""
import os
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch, gen
from znippy_amd import hip

n_poms = int(sys.argv[1]) if len(sys.argv) > 1 else 1400
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
ctx = hip.Context(0)


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return c.compress(data) + c.flush()


def count_symbols(s):
    """literal/length symbols (literals, matches, end-of-blocks) of a raw DEFLATE stream: a plain bit-by-bit canonical decoder"""
    pos = 0

    def bits(n):
        nonlocal pos
        v = 0
        for i in range(n):
            v |= ((s[pos >> 3] >> (pos & 7)) & 1) << i
            pos += 1
        return v

    def table(lens):
        cnt = [0] * 16
        for n in lens:
            cnt[n] += 1
        cnt[0] = 0
        offs = [0] * 16
        for n in range(1, 15):
            offs[n + 1] = offs[n] + cnt[n]
        sym = [0] * len(lens)
        for k, n in enumerate(lens):
            if n:
                sym[offs[n]] = k
                offs[n] += 1
        return cnt, sym

    def dec(t):
        cnt, sym = t
        code = first = index = 0
        for n in range(1, 16):
            code |= bits(1)
            if code - cnt[n] < first:
                return sym[index + code - first]
            index += cnt[n]
            first = (first + cnt[n]) << 1
            code <<= 1
        raise ValueError("bad code")
    lext = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
    symbols = 0
    while True:
        final, kind = bits(1), bits(2)
        if kind == 0:
            pos = (pos + 7) & ~7
            n = bits(16); bits(16)
            pos += 8 * n
        else:
            if kind == 1:
                ll, dd = table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), table([5] * 32)
            else:
                hlit, hdist, hclen = bits(5) + 257, bits(5) + 1, bits(4) + 4
                cl = [0] * 19
                for k in [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15][:hclen]:
                    cl[k] = bits(3)
                ct, lens = table(cl), []
                while len(lens) < hlit + hdist:
                    v = dec(ct)
                    if v < 16:
                        lens.append(v)
                    elif v == 16:
                        lens += [lens[-1]] * (3 + bits(2))
                    else:
                        lens += [0] * (3 + bits(3) if v == 17 else 11 + bits(7))
                ll, dd = table(lens[:hlit]), table(lens[hlit:])
            while True:
                v = dec(ll)
                symbols += 1
                if v == 256:
                    break
                if v > 256:
                    bits(lext[v - 257])
                    d = dec(dd)
                    bits(0 if d < 4 else (d - 2) >> 1)
        if final:
            return symbols


def to_batch(datas, strategy=zlib.Z_DEFAULT_STRATEGY):
    streams = [deflate(d, 6, strategy) for d in datas]
    off, pos = [], 1
    for s in streams:
        off.append(pos)
        pos = (pos + len(s)) | 1
    src = np.zeros(pos + 64, np.uint8)
    for s, o in zip(streams, off):
        src[o:o + len(s)] = np.frombuffer(s, np.uint8)
    return dict(datas=datas, streams=streams, off=off, d_src=torch.from_numpy(src).cuda(), d_out=torch.zeros(sum(len(d) for d in datas) + 64, dtype=torch.uint8, device="cuda"),
                crc=[zlib.crc32(d) for d in datas])


def gpu(b):
    wall, kt = [], None
    for _ in range(rounds + 1):
        torch.cuda.synchronize(); ctx.sync()
        t = time.perf_counter()
        st, crc = ctx.inflate_batch(b["d_src"], b["off"], [len(s) for s in b["streams"]], b["d_out"], [len(d) for d in b["datas"]], crc32=b["crc"])
        wall.append(time.perf_counter() - t)
        assert not st.any(), st[st != 0]
        kt = dict(ctx.kernel_times())
    wall = sorted(wall[1:])
    return wall[0] * 1e3, wall[len(wall) // 2] * 1e3, kt


def cpu_one(s):
    d = zlib.decompressobj(-15)
    out = d.decompress(s)
    return zlib.crc32(out)


def cpu(b, threads):
    best = 1e9
    with ThreadPoolExecutor(threads) as ex:
        for _ in range(rounds):
            t = time.perf_counter()
            if threads == 1:
                got = [cpu_one(s) for s in b["streams"]]
            else:
                got = list(ex.map(cpu_one, b["streams"], chunksize=max(1, len(b["streams"]) // (4 * threads))))
            best = min(best, time.perf_counter() - t)
            assert got == b["crc"]
    return best * 1e3


def report(name, b):
    best, med, kt = gpu(b)
    c16, c1 = cpu(b, 16), cpu(b, 1)
    n_in, n_out = sum(len(s) for s in b["streams"]), sum(len(d) for d in b["datas"])
    print(f"{name}: {len(b['datas'])} entries, {n_in} -> {n_out} bytes | call {best:.3f} ms (median {med:.3f}) | inflate {kt['inflate']:.3f} ms, inflate_crc {kt['inflate_crc']:.3f} ms"
          f" | zlib 16 threads {c16:.3f} ms, 1 thread {c1:.3f} ms | call / zlib16 = {best / c16:.2f}")
    return kt


print(f"device {torch.cuda.get_device_name(0)}  n_poms {n_poms}  rounds {rounds}  cpus used by the zlib side: 16 threads of {os.cpu_count()}")
poms = [gen.text(1024 + (i % 8) * 1024 + i % 97)[i % 97:] for i in range(n_poms)]
pb = to_batch(poms)
kt = report("poms", pb)
sample = list(range(0, n_poms, max(1, n_poms // 40)))
sym = sum(count_symbols(pb["streams"][i]) for i in sample) * sum(len(d) for d in poms) / sum(len(poms[i]) for i in sample)
print(f"poms: ~{sym / 1e6:.2f} M symbols (sample of {len(sample)}), {sym / (kt['inflate'] * 1e-3) / 1e6:.1f} M symbols/s over the batch")

words = [gen.pseudo_text(1024 + (i % 8) * 1024, seed=i % 50)[i % 31:] for i in range(n_poms)]
wb = to_batch(words)
kt = report("poms of word soup", wb)
sample = list(range(0, n_poms, max(1, n_poms // 40)))
sym = sum(count_symbols(wb["streams"][i]) for i in sample) * sum(len(d) for d in words) / sum(len(words[i]) for i in sample)
print(f"poms of word soup: ~{sym / 1e6:.2f} M symbols (sample of {len(sample)}), {sym / (kt['inflate'] * 1e-3) / 1e6:.1f} M symbols/s over the batch")

sizes = [100 << 10, 200 << 10, 400 << 10, 800 << 10, 1 << 20, 3 << 19, 2 << 20]
big = [gen.pseudo_text(n, seed=100 + k) for k, n in enumerate(sizes)]
bb = to_batch(big)
report("big set", bb)
per_byte = count_symbols(bb["streams"][0]) / sizes[0]
print(f"one entry alone = one wave (symbols from the {sizes[0] >> 10} KiB entry: {per_byte:.3f} per content byte):")
for d in big:
    one = to_batch([d])
    best, med, k1 = gpu(one)
    c1 = cpu(one, 1)
    print(f"  {len(d) >> 10:5d} KiB: call {best:.3f} ms, inflate {k1['inflate']:.3f} ms, inflate_crc {k1['inflate_crc']:.3f} ms, "
          f"{per_byte * len(d) / (k1['inflate'] * 1e-3) / 1e6:.2f} M symbols/s per wave, {len(d) / (k1['inflate'] * 1e-3) / 1e6:.1f} MB/s | zlib 1 thread {c1:.3f} ms"
          f" | wave / zlib = {k1['inflate'] / c1:.1f}")
for n in (1 << 10, 4 << 10, 16 << 10, 64 << 10):
    one = to_batch([gen.pseudo_text(n, seed=5)])
    best, med, k1 = gpu(one)
    print(f"  {n >> 10:5d} KiB: call {best:.3f} ms, inflate {k1['inflate']:.3f} ms | zlib 1 thread {cpu(one, 1):.4f} ms")
# literals only (Z_HUFFMAN_ONLY: one symbol per byte) and long matches only (zeros: 258 bytes per symbol): the two ends of a symbol's cost
for name, d, strategy in (("literals only", gen.pseudo_text(256 << 10, seed=9), zlib.Z_HUFFMAN_ONLY), ("zeros", bytes(4 << 20), zlib.Z_DEFAULT_STRATEGY)):
    one = to_batch([d], strategy)
    n_sym = count_symbols(one["streams"][0])
    best, med, k1 = gpu(one)
    print(f"  {name}, {len(d) >> 10} KiB alone: inflate {k1['inflate']:.3f} ms, {n_sym} symbols, {k1['inflate'] * 1e6 / n_sym:.0f} ns per symbol | zlib 1 thread {cpu(one, 1):.3f} ms")
ctx.close()

# the archive call: n_poms jars (a stored 64 KiB class blob, a deflated pom of 1-8 KiB of word soup, a properties file), archived once with the
# jars stored (the extension rule) and once with no_skip (compressed chunks); znippy_archive_extract_zip_entries for all of them against
# zipfile over the same jars as files (page cache warm on both sides: the archive and the jars were just written)
import io, shutil, tempfile, zipfile
from znippy_amd import host
tmp = tempfile.mkdtemp(prefix="inflate_report_")
try:
    paths = []
    for i in range(n_poms):
        b = io.BytesIO()
        with zipfile.ZipFile(b, "w") as zf:
            zf.writestr(zipfile.ZipInfo("g/a/C.class"), gen.incompressible(i % 13, 64 << 10), zipfile.ZIP_STORED)
            zf.writestr(zipfile.ZipInfo("META-INF/maven/g/a/pom.xml"), words[i], zipfile.ZIP_DEFLATED)
            zf.writestr(zipfile.ZipInfo("META-INF/maven/g/a/pom.properties"), b"version=1\n", zipfile.ZIP_STORED)
        rel = f"repo/{i % 37}/a-{i}.jar"
        os.makedirs(os.path.dirname(os.path.join(tmp, "in", rel)), exist_ok=True)
        with open(os.path.join(tmp, "in", rel), "wb") as f:
            f.write(b.getvalue())
        paths.append(rel)

    def zip_one(rel):
        with zipfile.ZipFile(os.path.join(tmp, "in", rel)) as zf:
            return zf.read("META-INF/maven/g/a/pom.xml")
    for no_skip in (False, True):
        arc = os.path.join(tmp, f"a{int(no_skip)}.znippy")
        host.compress_dir(os.path.join(tmp, "in"), arc, no_skip)
        a = host.ZnippyArchive.open(arc)
        t_call = []
        for _ in range(4):
            t = time.perf_counter()
            got, st = a.extract_zip_entries(paths, "pom.xml")
            t_call.append(time.perf_counter() - t)
        assert not any(st) and got == words
        a.close()
        print(f"archive of {n_poms} jars ({os.path.getsize(arc) >> 20} MiB, jars {'compressed' if no_skip else 'stored'}): extract_zip_entries first call {t_call[0] * 1e3:.1f} ms, "
              f"best of the next three {min(t_call[1:]) * 1e3:.1f} ms")
    with ThreadPoolExecutor(16) as ex:
        t = time.perf_counter(); got = list(ex.map(zip_one, paths)); t16 = time.perf_counter() - t
    t = time.perf_counter(); got1 = [zip_one(p) for p in paths]; t1 = time.perf_counter() - t
    assert got == words and got1 == words
    print(f"zipfile over the same jars as files: 16 threads {t16 * 1e3:.1f} ms, 1 thread {t1 * 1e3:.1f} ms")
finally:
    shutil.rmtree(tmp, ignore_errors=True)
