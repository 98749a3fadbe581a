"""The encoder's cross-block window (znippy_ctx_set_window_log) at windows 0, 17 and 23, level 19, on three corpora:
workload c3 (2 GiB of text in 8 MiB rounds, made on the device), the image's shared objects and its text files
(workloads.image_corpus).  Per corpus and window: ratio, encode ms (best of 3) and decode+verify ms (best of 2) of the
whole table, with the output compared to the input, and a sample of frames checked by libzstd.
Usage: python tools/window_report.py [binary_cap_MB] [text_cap_MB]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import workloads
from znippy_amd import hip

WINDOWS = (0, 17, 23)


def corpora():
    cap_bin = float(sys.argv[1]) * 1e6 if len(sys.argv) > 1 else 120e6
    cap_txt = float(sys.argv[2]) * 1e6 if len(sys.argv) > 2 else 64e6
    L = workloads.layout("c3")
    lens = L["lens"]
    yield "c3", lens, L["gen"](torch, 0, int(lens.sum()))
    for kind, cap in (("binary", cap_bin), ("text", cap_txt)):
        ents = workloads.image_corpus(kind, cap)
        lens = np.array([len(e) for e in ents], np.uint64)
        yield kind, lens, torch.from_numpy(np.frombuffer(b"".join(ents), np.uint8).copy()).cuda()


def main():
    for name, lens, d_in in corpora():
        total = int(lens.sum())
        offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
        d_src = torch.cat([d_in.reshape(-1)[:total], torch.zeros(64, dtype=torch.uint8, device="cuda")])
        multi = int((lens > 128 * 1024).sum())
        print(f"[{name}] {len(lens)} rounds, {total / 1e6:.1f} MB, {multi} of them longer than one block", flush=True)
        for wl in WINDOWS:
            ctx = hip.Context(0)
            ctx.set_level(19)
            ctx.set_window_log(wl)
            rt = hip.RoundTable(ctx, offs, lens)
            d_blob = torch.zeros(rt.blob_bound() + 64, dtype=torch.uint8, device="cuda")
            te = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                enc = rt.encode_hash(d_src, d_blob)
                te.append(time.perf_counter() - t0)
            enc = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in enc.items()}
            blob_bytes = int(enc["blob_size"].sum())
            # libzstd on a sample: the four longest rounds and ~40 spread over the table
            sample = sorted(set(np.argsort(lens)[-4:].tolist() + list(range(0, len(lens), max(1, len(lens) // 40)))))
            bad = 0
            for i in sample:
                o, s, u0, n = int(enc["blob_offset"][i]), int(enc["blob_size"][i]), int(offs[i]), int(lens[i])
                f = d_blob[o:o + s].cpu().numpy().tobytes()
                try:
                    ok = workloads.libzstd_decompress(f, max(n, 1)) == d_src[u0:u0 + n].cpu().numpy().tobytes()
                except Exception:
                    ok = False
                bad += 0 if ok else 1
            rows = hip.RowTable(ctx, enc["blob_offset"], enc["blob_size"], lens, offs, None, enc["checksum"])
            d_out = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")
            td = []
            for _ in range(2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                c, _, _ = rows.decode_verify(d_blob, d_out)
                td.append(time.perf_counter() - t0)
            same = bool((d_out[:total] == d_src[:total]).all())
            print(f"[{name}] window {wl:2d}: ratio {blob_bytes / total:.4f}  encode {min(te) * 1e3:.1f} ms  "
                  f"decode+verify {min(td) * 1e3:.1f} ms  same={same} corrupt={c['corrupt_rows']} errors={c['decode_errors']}  "
                  f"libzstd bad {bad}/{len(sample)}", flush=True)
            rows.close()
            rt.close()
            ctx.close()
            del d_blob, d_out
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
