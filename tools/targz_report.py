"""znippy_targz_find_batch on generated crates: what early stop buys, against the two routes there were before it.
  crates  N gzip-compressed GNU-format tars (default N = 1,400) of 20 KiB - 2 MiB of content each: a .cargo_vcs_info.json, the Cargo.toml
          (1-4 KiB), then source files of the generators' text (tests/gen.py: word soup and xml-like text; there are no real crates to
          measure, so how much early stop buys on real ones is unmeasured).  Three sets: the manifest second (where cargo package puts
          it), last, and absent.
Per set: the call by the wall clock (best and median of `rounds`, the device idle in front), the targz_find and targz_gather kernel
times, the bytes inflated (`scanned`) beside the content bytes, and
  (a) tarfile (mode r:gz, which also stops reading at the member) over the same crates on a pool of 16 threads and on one thread
  (b) the device route without this call: znippy_inflate_batch of every whole stream, sized by ISIZE, one copy back, then a walk of
      the tars on the host (tests/targz_model.py's walk on 16 threads).
The tool measures and promises nothing; the tests assert none of it.
With --parent ROOT (a checkout of the parent commit with its library built) it then runs tools/inflate_report.py of ROOT and of this
tree alternately, twice each, and compares the `inflate` kernel times of the "poms" and "poms of word soup" lines: this build's must
lie within the spread of the parent's two runs (k_inflate now instantiates the shared decoder body with an empty hook).

Usage: python tools/targz_report.py [--n 1400] [--rounds 5] [--out profiles/targz_report.log] [--parent ROOT]"""
import argparse
import gzip
import io
import os
import re
import subprocess
import sys
import tarfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1400)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "targz_report.log"))
ap.add_argument("--parent", default=None)
args = ap.parse_args()
log = open(args.out, "w")


def say(line=""):
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()


import torch, gen  # noqa: E402
import targz_model as M  # noqa: E402
from znippy_amd import hip  # noqa: E402

SUFFIX = b"/Cargo.toml"
base = [gen.pseudo_text(2 << 20, seed=200 + k) for k in range(6)] + [gen.text(2 << 20)]


def manifest(i):
    deps = b"".join(b"dep%d = { version = \"%d.%d\" }\n" % (k, k % 7, i % 11) for k in range(160))
    return (b"[package]\nname = \"crate%d\"\nversion = \"1.0.%d\"\n\n[dependencies]\n" % (i, i) + deps)[:1024 + (i * 997) % 3072]


def make_crate(i, where):
    content = int(20480 * 100 ** ((i * 0.6180339887) % 1.0))   # 20 KiB .. 2 MiB, evenly spread over the logarithm
    b = io.BytesIO()
    with tarfile.open(fileobj=b, mode="w", format=tarfile.GNU_FORMAT) as tf:
        def add(name, data):
            ti = tarfile.TarInfo(f"crate{i}-1.0.{i}/{name}")
            ti.size = len(data)
            tf.addfile(ti, io.BytesIO(data))
        add(".cargo_vcs_info.json", b'{"git":{"sha1":"%040x"},"path_in_vcs":""}' % i)
        if where == "second":
            add("Cargo.toml", manifest(i))
        k, left = 0, content
        while left > 0:
            n = min(left, 4096 + (i * 7919 + k * 104729) % (96 << 10))
            src = base[(i + k) % len(base)]
            at = (i * 65537 + k * 8191) % (len(src) - n)
            add(f"src/m{k}.rs", src[at:at + n])
            left -= n
            k += 1
        if where == "last":
            add("Cargo.toml", manifest(i))
    tar = b.getvalue()
    return gzip.compress(tar, 6, mtime=0), len(tar)


def tarfile_one(crate):
    with tarfile.open(fileobj=io.BytesIO(crate), mode="r:gz") as tf:
        for ti in tf:
            if ti.isreg() and ti.name.encode().endswith(SUFFIX):
                return tf.extractfile(ti).read()
    return None


def timed_pool(fn, items, threads, rounds):
    best, got = 1e9, None
    with ThreadPoolExecutor(threads) as ex:
        for _ in range(rounds):
            t = time.perf_counter()
            got = [fn(x) for x in items] if threads == 1 else list(ex.map(fn, items, chunksize=max(1, len(items) // (4 * threads))))
            best = min(best, time.perf_counter() - t)
    return best * 1e3, got


def report(ctx, where):
    t0 = time.perf_counter()
    with ThreadPoolExecutor(16) as ex:
        made = list(ex.map(lambda i: make_crate(i, where), range(args.n)))
    crates, tar_len = [c for c, _ in made], [n for _, n in made]
    want = [manifest(i) if where != "absent" else None for i in range(args.n)]
    off, pos = [], 0
    for c in crates:
        off.append(pos)
        pos += len(c)
    src = np.frombuffer(b"".join(crates) + bytes(64), np.uint8)
    d_src = torch.from_numpy(src.copy()).cuda()
    lens = [len(c) for c in crates]
    say(f"set '{where}': {args.n} crates, {sum(lens)} compressed -> {sum(tar_len)} tar bytes (generated in {time.perf_counter() - t0:.1f} s)")
    # the new call
    d_out = torch.zeros(args.n * 4096 + 64, dtype=torch.uint8, device="cuda")
    wall, kt = [], None
    for _ in range(args.rounds + 1):
        torch.cuda.synchronize(); ctx.sync()
        t = time.perf_counter()
        st, oo, ol, scanned = ctx.targz_find_batch(d_src, off, lens, d_out, SUFFIX)
        wall.append(time.perf_counter() - t)
        kt = dict(ctx.kernel_times())
    img = d_out.cpu().numpy()
    for i in range(args.n):
        assert (st[i] == 0 and img[int(oo[i]):int(oo[i] + ol[i])].tobytes() == want[i]) if want[i] is not None else st[i] == M.E_NOENT, (i, st[i])
    wall = sorted(wall[1:])
    say(f"  targz_find_batch: call {wall[0] * 1e3:.3f} ms (median {wall[len(wall) // 2] * 1e3:.3f}) | targz_find {kt.get('targz_find', 0):.3f} ms, "
        f"targz_gather {kt.get('targz_gather', 0):.3f} ms | scanned {int(scanned.sum())} of {sum(tar_len)} tar bytes ({100 * int(scanned.sum()) / sum(tar_len):.2f} %)")
    # (a) tarfile
    t16, got = timed_pool(tarfile_one, crates, 16, max(1, args.rounds // 2))
    assert got == want
    t1, got = timed_pool(tarfile_one, crates, 1, 1)
    say(f"  (a) tarfile r:gz: 16 threads {t16:.1f} ms, 1 thread {t1:.1f} ms | call / tarfile16 = {wall[0] * 1e3 / t16:.3f}")
    # (b) inflate the whole streams, copy back, walk on the host
    isize = [int.from_bytes(c[-4:], "little") for c in crates]
    assert isize == tar_len
    u_off = np.concatenate([[0], np.cumsum(isize)[:-1]]).astype(np.uint64)
    d_tar = torch.zeros(sum(isize) + 64, dtype=torch.uint8, device="cuda")
    best = 1e9
    for _ in range(max(2, args.rounds // 2)):
        torch.cuda.synchronize(); ctx.sync()
        t = time.perf_counter()
        st2, _ = ctx.inflate_batch(d_src, [o + 10 for o in off], [n - 18 for n in lens], d_tar, isize)
        t_call = time.perf_counter() - t
        kt2 = dict(ctx.kernel_times())
        tars = d_tar.cpu().numpy()
        t_copy = time.perf_counter() - t - t_call
        views = [tars[int(o):int(o) + n].tobytes() for o, n in zip(u_off, isize)]
        with ThreadPoolExecutor(16) as ex:
            found = list(ex.map(lambda v: M.walk(v, True, b"", SUFFIX), views))
        total = time.perf_counter() - t
        assert not st2.any()
        if total < best:
            best, parts = total, (t_call, t_copy, total - t_call - t_copy)
    for i, (s, o, n, _) in enumerate(found):
        assert (s == 0 and views[i][o:o + n] == want[i]) if want[i] is not None else s == M.E_NOENT
    say(f"  (b) inflate_batch of the whole streams + copy back + host walk: {best * 1e3:.1f} ms (call {parts[0] * 1e3:.1f} incl. inflate {kt2['inflate']:.3f} and inflate_crc "
        f"{kt2['inflate_crc']:.3f}, copy {parts[1] * 1e3:.1f}, slicing and walk on 16 threads {parts[2] * 1e3:.1f}) | call / (b) = {wall[0] / best:.3f}")


ctx = hip.Context(0)
say(f"device {torch.cuda.get_device_name(0)}  n_crates {args.n}  rounds {args.rounds}  cpus used by the host side: 16 threads of {os.cpu_count()}")
for where in ("second", "last", "absent"):
    report(ctx, where)
ctx.close()

if args.parent:
    say()
    say("k_inflate, parent build against this build: tools/inflate_report.py, alternating, `inflate` kernel ms of the two pom lines")
    pat = re.compile(r"^(poms|poms of word soup): .*\| inflate ([0-9.]+) ms", re.M)
    runs = {"parent": [], "child": []}
    for k in range(2):
        for who, root in (("parent", os.path.abspath(args.parent)), ("child", ROOT)):
            r = subprocess.run([sys.executable, os.path.join(root, "tools", "inflate_report.py"), "1400", "5"], capture_output=True, text=True, cwd=root)
            if r.returncode != 0:
                say(f"  {who} run {k + 1} failed: rc={r.returncode} {r.stderr[-400:]}")
                sys.exit(1)
            got = {name: float(ms) for name, ms in pat.findall(r.stdout)}
            runs[who].append(got)
            say(f"  {who} run {k + 1}: poms {got['poms']:.3f} ms, poms of word soup {got['poms of word soup']:.3f} ms")
    for name in ("poms", "poms of word soup"):
        p, c = [x[name] for x in runs["parent"]], [x[name] for x in runs["child"]]
        inside = [min(p) <= v <= max(p) for v in c]
        side = "on the fast side" if max(c) < min(p) else "on the slow side" if min(c) > max(p) else "on both sides or one run only"
        say(f"  {name}: parent {min(p):.3f} .. {max(p):.3f} ms, this build {c[0]:.3f}, {c[1]:.3f} ms -> "
            f"{'inside the parent spread' if all(inside) else 'OUTSIDE the parent spread, ' + side} (this build / parent mean = {sum(c) / sum(p):.3f})")
log.close()
