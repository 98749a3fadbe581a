"""Static count of the 6 x 10 hash loop of k_fused_roles, as in profiles/roles_loop_static.txt: the device code of
csrc/fused_small.hip is compiled for gfx950 and disassembled, and the instructions between the header and the back edge of
the two-pass hash loop of each instantiation are counted.  "VALU" = every v_* instruction but v_readlane / v_readfirstlane /
v_writelane.  Registers and spills come from -Rpass-analysis=kernel-resource-usage.  Needs no GPU.

Usage: python tools/roles_loop_count.py [path/to/fused_small.hip] [extra hipcc flags, e.g. -DZN_R_WAVES=16 -DZN_R_SLOTS=32]"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "znippy_amd", "csrc")
args = sys.argv[1:]
src = args.pop(0) if args and not args[0].startswith("-") else os.path.join(CSRC, "fused_small.hip")
rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
hipcc = os.environ.get("HIPCC", os.path.join(rocm, "bin", "hipcc"))
objdump = os.path.join(rocm, "llvm", "bin", "llvm-objdump")

with tempfile.TemporaryDirectory() as tmp:
    obj = os.path.join(tmp, "fused_small.co")
    cmd = [hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "--no-gpu-bundle-output", "-I", CSRC,
           "-I", os.path.join(ROOT, "include"), "-Wno-unused-function", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", obj] + args
    rem = subprocess.run(cmd, check=True, capture_output=True, text=True).stderr
    dis = subprocess.run([objdump, "-d", obj], check=True, capture_output=True, text=True).stdout

res = {}
cur = None
for line in rem.splitlines():
    m = re.search(r"Function Name: (\S+)", line)
    if m:
        cur = m.group(1)
    m = re.search(r"remark:\s+(VGPRs|TotalSGPRs|VGPRs Spill|SGPRs Spill|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
    if m and cur:
        res.setdefault(cur, {})[m.group(1)] = int(m.group(2))

funcs = {}
name = None
for line in dis.splitlines():
    m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
    if m:
        name = m.group(1)
        funcs[name] = []
        continue
    m = re.match(r"^\s+(\S+)\s+(.*?)\s*// ([0-9A-F]+): ((?:[0-9A-F]{8} ?)+)", line)
    if m and name:
        funcs[name].append((int(m.group(3), 16), m.group(1), m.group(2), len(m.group(4).split())))


def valu(op):
    return op.startswith("v_") and not op.startswith(("v_readlane", "v_readfirstlane", "v_writelane"))


for fn, ins in funcs.items():
    if "k_fused_roles" not in fn:
        continue
    addr = {a: i for i, (a, _, _, _) in enumerate(ins)}
    best = None
    for i, (a, op, operands, dw) in enumerate(ins):
        if not op.startswith(("s_cbranch", "s_branch")):
            continue
        off = int(operands.split()[-1])
        off = off - 65536 if off >= 32768 else off
        tgt = a + 4 + 4 * off
        if tgt <= a and tgt in addr:
            body = ins[addr[tgt]:i + 1]
            nv = sum(1 for _, o, _, _ in body if valu(o))
            # the hash loop: two compressions of 678 VALU and little else (the loops around it hold it and much more)
            if 2 * 678 <= nv < 3 * 678 and (best is None or len(body) < len(best)):
                best = body
    kind = "<true>" if "Lb1" in fn else "<false>"
    r = res.get(fn, {})
    print(f"{fn}  {kind}")
    print(f"  registers: {r}")
    if best:
        nv = sum(1 for _, op, _, _ in best if valu(op))
        dv = sum(dw for _, op, _, dw in best if valu(op))
        print(f"  hash loop: {len(best)} instructions, {sum(dw for *_, dw in best)} dwords; VALU {nv} in {dv} dwords"
              f"  (per pass of two: {nv / 2:.1f} VALU, {dv / 2:.1f} VALU dwords, {nv / 2 - 678:.1f} other VALU)")
