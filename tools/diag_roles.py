"""Diagnostic: which rows does the role-split kernel get wrong (digest / bytes), and how are they distributed; then where its
waves spent their time in the last run (ramp, feed and tail of the hashers, the loader's waits and its first iteration:
ZNIPPY_DBG bit 32768 is set for the context, the kernel's geometry is the library's)."""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch, gen
import workloads
from znippy_amd import hip
n, sz = int(os.environ.get("N", 100000)), 10240
os.environ["ZNIPPY_DBG"] = str(int(os.environ.get("ZNIPPY_DBG", "0")) | 32768)  # the waves leave their clocks and waits
ctx = hip.Context(0)
chunk = gen.text(sz)
frame = np.frombuffer(workloads.libzstd_compress(chunk, 19), dtype=np.uint8)
fl = len(frame)
d_blobs = torch.from_numpy(np.concatenate([np.tile(frame, n), np.zeros(64, np.uint8)])).cuda()
want = np.frombuffer(ctx.blake3(chunk), dtype=np.uint8)
ck = np.tile(want, (n, 1))
rt = hip.RowTable(ctx, np.arange(n, dtype=np.uint64) * fl, np.full(n, fl, np.uint64), np.full(n, sz, np.uint64),
                  np.arange(n, dtype=np.uint64) * sz, None, ck)
d_out = torch.zeros(n * sz + 64, dtype=torch.uint8, device="cuda")
for rep in range(3):
    d_out.zero_()
    c, corrupt, status = rt.decode_verify(d_blobs, d_out)
    dg = rt.digests()
    bad = np.nonzero((dg != want[None, :]).any(axis=1))[0]
    ref = torch.from_numpy(np.frombuffer(chunk, dtype=np.uint8).copy()).cuda()
    bytes_bad = torch.nonzero((d_out[:n * sz].view(n, sz) != ref[None, :]).any(dim=1)).flatten().cpu().numpy()
    print(f"rep {rep}: counters {c['corrupt_rows']} corrupt, digest-bad {len(bad)}, bytes-bad {len(bytes_bad)}, status!=0 {int((status != 0).sum())}")
    if len(bad):
        tiles = bad // 6
        print("  bad rows head:", bad[:24].tolist())
        print("  row%6 hist:", np.bincount(bad % 6, minlength=6).tolist(), " tile%4 hist:", np.bincount(tiles % 4, minlength=4).tolist())
        ut, cnt = np.unique(tiles, return_counts=True)
        print("  bad tiles:", len(ut), " rows-per-bad-tile hist:", np.bincount(cnt, minlength=7).tolist())
        print("  group(=tile//4) count:", len(np.unique(tiles // 4)), " distinct digests among bad:", len(np.unique(dg[bad], axis=0)))
    if len(bytes_bad):
        print("  bytes-bad rows head:", bytes_bad[:24].tolist())
print(ctx.kernel_times())
print("shader GHz during the read kernel:", ctx.last_shader_ghz())


def wait_report(ctx):
    """Where the waves of the last run's role-split kernel spent their time (znippy_roles_wait_stats): per role the mean of
    each wait and its share of the waves' life; `gone` = from a wave's exit to the exit of its workgroup's last wave (the CU's
    registers and LDS are handed over only then), as a share of the workgroup's life."""
    geom, w = ctx.roles_wait_stats()
    print("geometry:", geom)
    if not len(w) or not w[0, 7]:
        print("no wait counters (the kernel did not run, or ZNIPPY_DBG bit 32768 is clear)")
        return
    W = geom["waves"]
    w = w[:int(w[0, 7]) * W].astype(np.float64).reshape(-1, W, 8)
    life, ticks = w[:, :, 0], w[:, :, 6] - w[:, :, 5]
    ghz = float(np.median(life[ticks > 0] / ticks[ticks > 0])) * 0.1
    us = lambda cyc: cyc / (ghz * 1e3)
    wg0, wg1 = w[:, :, 5].min(axis=1), w[:, :, 6].max(axis=1)
    k0, k1 = wg0.min(), wg1.max()
    print(f"workgroups {w.shape[0]} x {W} waves, shader clock {ghz:.3f} GHz, kernel {(k1 - k0) * 0.01:.1f} us from the first wave's start to the last wave's end")
    print(f"  workgroup life: mean {np.mean(wg1 - wg0) * 0.01:.1f} us, min {np.min(wg1 - wg0) * 0.01:.1f}, max {np.max(wg1 - wg0) * 0.01:.1f};"
          f" start after the kernel's: mean {np.mean(wg0 - k0) * 0.01:.1f} us, max {np.max(wg0 - k0) * 0.01:.1f};"
          f" end before the kernel's: mean {np.mean(k1 - wg1) * 0.01:.1f} us, max {np.max(k1 - wg1) * 0.01:.1f}")
    L, H = w[:, 0, :], w[:, 1:, :]
    hl = H[:, :, 0].sum()
    gone = (wg1[:, None] - H[:, :, 6]) * 0.01
    print(f"  hashers: life {us(H[:, :, 0].mean()):.1f} us, tiles {H[:, :, 4].mean():.2f} (min {H[:, :, 4].min():.0f}, max {H[:, :, 4].max():.0f})")
    for k, name in ((1, "ramp (before the first tile)"), (2, "feed (between tiles)"), (3, "tail (the wait that ends without a tile)")):
        print(f"    {name:42s} mean {us(H[:, :, k].mean()):7.2f} us  max {us(H[:, :, k].max()):7.2f} us  {H[:, :, k].sum() / hl * 100:5.2f} % of hasher wave time")
    print(f"    {'gone (exit to the workgroup end)':42s} mean {gone.mean():7.2f} us  max {gone.max():7.2f} us  {gone.sum() / ((wg1 - wg0).sum() * 0.01 * (W - 1)) * 100:5.2f} % of hasher slots x workgroup life")
    print(f"  loader: life {us(L[:, 0].mean()):.1f} us, iterations {L[:, 4].mean():.2f}")
    for k, name in ((1, "waits for a free group (gen)"), (2, "waits for its publish turn"), (3, "first iteration (start to first publish)")):
        print(f"    {name:42s} mean {us(L[:, k].mean()):7.2f} us  max {us(L[:, k].max()):7.2f} us  {L[:, k].sum() / L[:, 0].sum() * 100:5.2f} % of loader wave time")
    it = L[:, 4] > 1
    if it.any():
        busy = L[it, 0] - L[it, 1] - L[it, 2]
        print(f"    an iteration without its waits: mean {us((busy / L[it, 4]).mean()):.2f} us")


if hasattr(ctx.L, "znippy_roles_wait_stats"):  # (an older build of the library, run for comparison, has none)
    wait_report(ctx)
if os.environ.get("UBENCH"):
    print("blake3 pass ns:", ctx.blake3_pass_ns(), "at GHz", ctx.ubench_ghz)
