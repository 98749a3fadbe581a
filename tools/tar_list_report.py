"""znippy_tar_list_batch on generated tars: the call and its stages against Python's tarfile on one thread and on a pool of 16
(tars are independent; tarfile holds the GIL, so the pool shows what a Python caller gets, not what 16 cores could do) and against
znippy_tar_list_members, the serial C++ listing, on bytes already on the host.
Rounds are interleaved A, B, A': the two series of the call give its own spread (A/A), which is the margin of every ratio beside it.
Figures are medians of the wall clock of the call, the device idle in front and the tars already in device memory; stage times are
the kernel times of the last call.  The scan rate is also given as a share of the copy rate of the store path that
profiles/decode_only_report.log records (copy_stored, 2546 GB/s written).
  1. 1,400 crate-like tars of 20-200 KiB
  2. one tar above 256 MiB with 3,000 members (beyond the Infinity Cache: the scan figure is a memory figure)
  3. one tar of 100,000 empty and tiny members
  4. the host call (znippy_archive_list_tar_members) on .tar, .tar.gz and .tar.bz2 files of an archive
The tool measures and promises nothing; the tests assert none of it.

Usage: python tools/tar_list_report.py [--rounds 5] [--out profiles/tar_list_report.log]"""
import argparse
import bz2
import ctypes as C
import gzip
import io
import os
import statistics
import sys
import tarfile
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tar_list_report.log"))
args = ap.parse_args()
log = open(args.out, "w")


def say(line=""):
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()


import torch, gen  # noqa: E402
from znippy_amd import hip, host  # noqa: E402

med = statistics.median
COPY_GBS = 2546.0  # profiles/decode_only_report.log: copy_stored, c2store
TEXT = gen.pseudo_text(1 << 20, seed=700)


def make_tar(members, fmt=tarfile.GNU_FORMAT):
    b = io.BytesIO()
    with tarfile.open(fileobj=b, mode="w", format=fmt) as tf:
        for name, size, at in members:
            ti = tarfile.TarInfo(name)
            ti.size = size
            tf.addfile(ti, io.BytesIO(TEXT[at:at + size]))
    return b.getvalue()


def crate(k):
    """a crate-like tar of 20-200 KiB: a manifest, a lock file, sources of mixed sizes, a long path now and then"""
    rng = np.random.default_rng(1000 + k)
    want = int(rng.integers(20 << 10, 200 << 10))
    members, total, j = [("crate-%d-0.1.0/Cargo.toml" % k, 400 + k % 300, k % 1000)], 0, 0
    while total < want:
        size = int(min(rng.integers(200, 24 << 10), want - total + 200))
        deep = "/" + "module_with_a_long_name_%d" % j * 4 if j % 11 == 10 else ""
        members.append(("crate-%d-0.1.0/src%s/f%d.rs" % (k, deep, j), size, int(rng.integers(0, (1 << 20) - size))))
        total += size + 512
        j += 1
    return make_tar(members, tarfile.PAX_FORMAT if k % 3 == 0 else tarfile.GNU_FORMAT)


def tarfile_list(t):
    with tarfile.open(fileobj=io.BytesIO(t), mode="r:") as tf:
        return sum(1 for ti in tf if ti.isreg())


L = hip._lib.lib()
L.znippy_tar_list_members.argtypes = [C.c_void_p, C.c_uint64, C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                      C.c_void_p, C.c_void_p, C.c_void_p]


class HostLister:
    """znippy_tar_list_members with lists that hold everything"""
    def __init__(self, tars, members):
        self.arrs = [np.frombuffer(t, dtype=np.uint8) for t in tars]
        self.members = np.zeros(max(members, 1), dtype=hip.TAR_MEMBER)
        self.names = np.zeros(max(len(t) for t in tars), dtype=np.uint8)
        self.n = (C.c_uint64 * 3)()

    def run(self):
        total = 0
        for a in self.arrs:
            rc = L.znippy_tar_list_members(a.ctypes.data, a.size, b"", 0, b"", 0, self.members.ctypes.data, self.members.size, self.names.ctypes.data,
                                           self.names.size, C.byref(self.n, 0), C.byref(self.n, 8), C.byref(self.n, 16))
            assert rc == 0, rc
            total += self.n[0]
        return total


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def workload(ctx, title, tars, contents, base_rounds):
    total = sum(len(t) for t in tars)
    d_tar = torch.from_numpy(np.frombuffer(b"".join(tars) + bytes(64), dtype=np.uint8).copy()).cuda()
    off = np.concatenate([[0], np.cumsum([len(t) for t in tars])[:-1]]).astype(np.uint64)
    ln = [len(t) for t in tars]
    st, first, members, names, nb, ob = ctx.tar_list_batch(d_tar, off, ln)
    assert (st == 0).all(), st
    n_members = int(first[-1])
    d_out = torch.zeros(ob + 64, dtype=torch.uint8, device="cuda") if contents else None
    rounds_chain = max(int(np.ceil(np.log2(max(ln) // 512 + 1))), 0)
    say(f"{title}  ({len(tars)} tars, {total / 2**20:.1f} MiB, {n_members} members, {nb} name bytes, {ob / 2**20:.1f} MiB of contents; "
        f"{total // 512 + len(tars)} nodes, {rounds_chain} chain rounds)")

    def listing():
        return ctx.tar_list_batch(d_tar, off, ln, members_cap=n_members, names_cap=nb)

    def measure():
        return ctx.tar_list_batch(d_tar, off, ln, measure=True)

    def extract():
        return ctx.tar_list_batch(d_tar, off, ln, d_out=d_out, members_cap=n_members, names_cap=nb)

    for _ in range(2):
        listing()
    a, b, a2, m, e = [], [], [], [], []
    for _ in range(args.rounds):
        a.append(timed(listing)[0]); b.append(timed(measure)[0]); a2.append(timed(listing)[0])
        if contents:
            e.append(timed(extract)[0])
    listing()
    stages = ctx.kernel_times()
    spread = abs(med(a) - med(a2)) / med(a) * 100
    say(f"  A/A: list call ms (median of {args.rounds}) A {med(a):.3f}  A' {med(a2):.3f}  spread {spread:.2f} %")
    say(f"  call ms: list {med(a):.3f} ({total / med(a) / 1e6:.1f} GB/s of tar, {n_members / med(a) / 1e3:.2f} M members/s)  measure mode {med(b):.3f}" +
        (f"  list + contents {med(e):.3f}" if contents else ""))
    ksum = sum(ms for _, ms in stages)
    say("  kernel ms of the list call: " + "  ".join(f"{name} {ms:.4f}" for name, ms in stages) + f"  sum {ksum:.4f}  (host and copies: {med(a) - ksum:.3f})")
    scan = dict(stages)["tar_scan"]
    say(f"  scan: {total / scan / 1e6:.0f} GB/s read = {total / scan / 1e6 / COPY_GBS * 100:.1f} % of the store path's copy rate ({COPY_GBS:.0f} GB/s)")
    if contents:
        extract()
        say("  kernel ms with contents: " + "  ".join(f"{name} {ms:.4f}" for name, ms in ctx.kernel_times()))
    # baselines
    one, pool, hostc = [], [], []
    hl = HostLister(tars, n_members)
    with ThreadPoolExecutor(16) as ex:
        for _ in range(base_rounds):
            ms, r = timed(lambda: sum(tarfile_list(t) for t in tars)); one.append(ms)
            assert r == n_members
            ms, r = timed(lambda: sum(ex.map(tarfile_list, tars))); pool.append(ms)
            ms, r = timed(hl.run); hostc.append(ms)
            assert r == n_members
    say(f"  baselines ms (median of {base_rounds}): tarfile, 1 thread {med(one):.1f}  tarfile, 16 threads {med(pool):.1f}  znippy_tar_list_members (host bytes) {med(hostc):.3f}")
    say(f"  list call against: tarfile x 1 {med(one) / med(a):.0f}x  tarfile x 16 {med(pool) / med(a):.0f}x  host listing {med(hostc) / med(a):.2f}x"
        f"  (H2D of the tars, not in any figure: {total / 2**20:.0f} MiB)")
    say()
    del d_tar, d_out
    torch.cuda.empty_cache()


def host_call(crates):
    say("host call: znippy_archive_list_tar_members on an archive of .tar, .tar.gz and .tar.bz2 files (150 crate-like tars, 50 of each)")
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "in")
        os.makedirs(src)
        paths = {"tar": [], "tar.gz": [], "tar.bz2": []}
        for k, t in enumerate(crates[:150]):
            ext = ("tar", "tar.gz", "tar.bz2")[k % 3]
            data = t if ext == "tar" else gzip.compress(t, 6) if ext == "tar.gz" else bz2.compress(t, 9)
            with open(os.path.join(src, f"c{k}.{ext}"), "wb") as f:
                f.write(data)
            paths[ext].append(f"c{k}.{ext}")
        out = os.path.join(d, "a.znippy")
        host.compress_dir(src, out)
        a = host.ZnippyArchive.open(out)
        try:
            for what, sel in list(paths.items()) + [("all three", [p for v in paths.values() for p in v])]:
                a.list_tar_members(sel)
                names, cont = [], []
                for _ in range(args.rounds):
                    ms, r = timed(lambda: a.list_tar_members(sel)); names.append(ms)
                    assert all(s == 0 for s, _ in r)
                    cont.append(timed(lambda: a.list_tar_members(sel, contents=True))[0])
                n_members = sum(len(m) for _, m in r)
                say(f"  {what:9s} {len(sel):3d} files, {n_members} members: list ms {med(names):.2f}  list + contents ms {med(cont):.2f}"
                    "  (both: a measuring call, then the call with exact buffers)")
        finally:
            a.close()
    say()


def main():
    ctx = hip.Context(0)
    say(f"tar_list_report: {torch.cuda.get_device_name(0)}, rounds {args.rounds}")
    say()
    t0 = time.perf_counter()
    crates = [crate(k) for k in range(1400)]
    big = make_tar([("big-1.0/data/part%04d.bin" % k, 88_000 + 13 * k, (k * 7919) % ((1 << 20) - 130_000)) for k in range(3000)])
    assert len(big) > 256 << 20
    tiny = make_tar([("tiny/%06d" % k, k % 3, k % 1000) for k in range(100_000)])
    say(f"(generated in {time.perf_counter() - t0:.1f} s)")
    say()
    workload(ctx, "1. 1,400 crate-like tars", crates, True, min(args.rounds, 3))
    workload(ctx, "2. one tar above 256 MiB", [big], True, min(args.rounds, 3))
    workload(ctx, "3. one tar of 100,000 empty and tiny members", [tiny], False, min(args.rounds, 2))
    host_call(crates)
    ctx.close()


main()
