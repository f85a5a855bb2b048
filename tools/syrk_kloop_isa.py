#!/usr/bin/env python3
"""What the compiler made of the K loop of syrk_lower_body (csrc/dense_kernels.hip): cross-compiles the file for gfx950 with the flags of piqp_amd/build.py (no
GPU needed) and prints, for every k_syrk_* kernel,
  - the register table (VGPR / SGPR / scratch / waves per SIMD by registers), as recorded in profiles/syrk_kloop_before_after.txt section 5;
  - the loops that hold matrix operations, reduced to what decides whether the prefetch works: labels and branches, global / scalar loads, every s_waitcnt, the LDS
    traffic, the runs of matrix operations, 64-bit vector address arithmetic, v_mul_f64 / v_mov_b64, the barrier.
The property to read off (profiles/syrk_kloop_before_after.txt section 4): on the fast path no `s_waitcnt vmcnt(N)` that covers the operand loads of the stage
just requested stands between those loads and the first matrix operation behind them.  The source leans on two empty asm statements (scalar-base addressing,
vector weight loads), so run this again after a compiler change.

usage: python3 tools/syrk_kloop_isa.py [--kernel SUBSTRING] [--keep DIR]"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "piqp_amd", "csrc", "dense_kernels.hip")
KEEP = re.compile(r"^\s+(s_cbranch\S*|s_branch|s_barrier|s_waitcnt|global_load\S*|global_store\S*|s_load\S*|scratch_\S+|ds_read\S*|ds_write\S*|v_mfma\S*|v_mul_f64|v_mov_b64\S*|"
                  r"v_mad_[iu]64\S*|v_lshl_add_u64|s_endpgm)\b")
RUNS = ("v_mfma", "ds_read", "ds_write", "v_mul_f64", "v_mov_b64")


def demangle(name):
    try:
        return subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip().split("(")[0].replace("void ", "").replace("pq::dense::", "")
    except OSError:
        return name


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", default="k_syrk_lower<0, 2, 2>", help="kernel whose loops are listed (substring of the demangled name; 'all' = every k_syrk kernel)")
    ap.add_argument("--keep", default=None, help="directory that keeps the .s file")
    args = ap.parse_args()
    out = args.keep or tempfile.mkdtemp(prefix="syrk_isa_")
    os.makedirs(out, exist_ok=True)
    asm = os.path.join(out, "dense_kernels.s")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-x", "hip", "-ffp-contract=on", "--cuda-device-only", "-S",
           "-Rpass-analysis=kernel-resource-usage", SRC, "-o", asm]
    cp = subprocess.run(cmd, capture_output=True, text=True)
    if cp.returncode != 0:
        sys.exit(cp.stderr[-2000:])
    # register table
    table, cur = {}, None
    for ln in cp.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = m.group(1)
            table[cur] = {}
        m = re.search(r"remark:\s+(TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", ln)
        if m and cur:
            table[cur][m.group(1)] = int(m.group(2))
    names = {k: demangle(k) for k in table if "k_syrk" in k}
    print("| kernel | VGPR | SGPR | scratch B/lane | waves/SIMD by registers |\n|---|---|---|---|---|")
    for k, d in names.items():
        t = table[k]
        print(f"| {d} | {t['VGPRs']} | {t['TotalSGPRs']} | {t['ScratchSize [bytes/lane]']} | {t['Occupancy [waves/SIMD]']} |")
    # loops with matrix operations
    lines = open(asm).read().splitlines()
    for k, d in names.items():
        if args.kernel != "all" and args.kernel not in d:
            continue
        start = lines.index(k + ":") if (k + ":") in lines else next(i for i, ln in enumerate(lines) if ln.startswith(k + ":"))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))  # (not the first s_endpgm: kernels return early)
        body = lines[start:end + 1]
        # a loop = its header block and every block the compiler marks `in Loop: Header=<that block>`, in layout order (a rotated loop has blocks in front of its header)
        blocks, curb = [], None
        for ln in body:
            if re.match(r"^\.LBB\d+_\d+:", ln):
                curb = [ln]
                blocks.append(curb)
            elif curb is not None:
                curb.append(ln)
        for blk in blocks:
            m = re.match(r"^(\.LBB\d+_\d+):.*Loop Header", blk[0])
            if not m:
                continue
            tag = "Header=" + m.group(1)[2:] + " "
            loop = [x for bb in blocks if bb is blk or tag in bb[0] + " " for x in bb]
            if not any("v_mfma" in x for x in loop):
                continue
            i, last, body_l = 0, len(loop) - 1, loop
            print(f"\n== {d}: loop {m.group(1)} ({last - i + 1} lines)")
            prev, count = None, 0
            for x in body_l:
                if re.match(r"^\.LBB", x):
                    key, text = None, x.split(";")[0].rstrip()
                else:
                    mm = KEEP.match(x)
                    if not mm:
                        continue
                    key, text = mm.group(1), x.split(";")[0].rstrip()
                run = key is not None and key.startswith(RUNS)
                if run and prev == key:
                    count += 1
                    continue
                if count:
                    print(f"\t    ... {count} more")
                count = 0
                print(text)
                prev = key if run else None
            if count:
                print(f"\t    ... {count} more")


if __name__ == "__main__":
    main()
