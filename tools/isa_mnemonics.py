"""Static mnemonic counts per kernel of an AMDGPU .s file: what an argument table costs (lane reads / writes of spilled SGPRs,
hazard nops, scalar loads, scratch traffic) beside the fp64 arithmetic, which plumbing must not change.
   python tools/isa_mnemonics.py file.s [kernel-substring ...]
   python tools/isa_mnemonics.py --census DIR      (the tables of tools/kernarg_census.sh from its <stem>_<f64|f32>.s / .remarks)"""
import re
import subprocess
import sys

COLS = ("valu", "readlane", "writelane", "s_nop", "s_load", "scratch", "add_f64", "mul_f64", "fma_f64", "div_f64")


def classify(op):
    out = []
    if op.startswith("v_"):
        out.append("valu")
    if op == "v_readlane_b32":
        out.append("readlane")
    elif op == "v_writelane_b32":
        out.append("writelane")
    elif op == "s_nop":
        out.append("s_nop")
    elif op.startswith("s_load_") or op.startswith("s_buffer_load_"):
        out.append("s_load")
    elif op.startswith("scratch_"):
        out.append("scratch")
    elif op.startswith("v_add_f64"):
        out.append("add_f64")
    elif op.startswith("v_mul_f64"):
        out.append("mul_f64")
    elif op.startswith("v_fma_f64") or op.startswith("v_fmac_f64"):
        out.append("fma_f64")
    elif op.startswith("v_div_") and "f64" in op:
        out.append("div_f64")
    return out


def census(path):
    cur, data = None, {}
    for ln in open(path):
        m = re.match(r"^(_Z\w+):\s*; @", ln)
        if m:
            cur = m.group(1)
            data[cur] = dict.fromkeys(COLS, 0)
            continue
        if cur is None or not ln.startswith("\t") or ln.startswith("\t."):
            continue
        parts = ln.split()
        if not parts:
            continue
        if parts[0] == "s_endpgm":
            cur = None
            continue
        for c in classify(parts[0]):
            data[cur][c] += 1
    return data


def demangle(names):
    try:
        out = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.split("\n")
        return [re.sub(r"\(.*", "", o) for o in out[: len(names)]]
    except (OSError, subprocess.CalledProcessError):
        return names


KERNARG_KERNELS = ("k_fvt_scalars", "k_divdamp_fused")  # the kernels that read their argument table in place


def resource_usage(path):
    """[(mangled name, [TotalSGPRs, VGPRs, AGPRs, Scratch, Occupancy, SGPRspill, VGPRspill, LDS])] from the compiler's remarks."""
    rows, cur = [], None
    keys = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill",
            "LDS Size [bytes/block]")
    for ln in open(path):
        m = re.search(r"remark: Function Name: (\S+)", ln)
        if m:
            cur = (m.group(1), {})
            rows.append(cur)
            continue
        m = re.search(r"remark:\s+([^:]+): (\d+) \[-Rpass", ln)
        if m and cur is not None and m.group(1) in keys:
            cur[1][m.group(1)] = int(m.group(2))
    return [(n, [d.get(k, 0) for k in keys]) for n, d in rows]


def census_tables(d):
    import glob
    import os

    print("columns: TotalSGPRs VGPRs AGPRs Scratch[bytes/lane] Occupancy[waves/SIMD] SGPRspill VGPRspill LDS[bytes/block]")
    stems = sorted(os.path.basename(f)[:-8] for f in glob.glob(os.path.join(d, "*.remarks")))
    for stem in stems:
        rows = resource_usage(os.path.join(d, stem + ".remarks"))
        for (n, v), pretty in zip(rows, demangle([n for n, _ in rows])):
            print(f"{stem:12s} {v[0]:5d} {v[1]:4d} {v[2]:3d} {v[3]:5d} {v[4]:2d} {v[5]:4d} {v[6]:4d} {v[7]:6d}  {pretty}")
    print()
    print("static counts -- columns: " + " ".join(COLS) + "  (div_f64: v_div_scale / fmas / fixup, 4 per division)")
    for stem in stems:
        data = census(os.path.join(d, stem + ".s"))
        names = [k for k in data if any(w in k for w in KERNARG_KERNELS)]
        for k, pretty in zip(names, demangle(names)):
            print(f"{stem:12s} " + " ".join(f"{data[k][c]:6d}" for c in COLS) + "  " + pretty)


if __name__ == "__main__":
    if sys.argv[1] == "--census":
        census_tables(sys.argv[2])
        sys.exit(0)
    data = census(sys.argv[1])
    wants = sys.argv[2:] or [""]
    names = [k for k in data if any(w in k for w in wants)]
    print("columns: " + " ".join(COLS) + "  (v_div_* counts v_div_scale / fmas / fixup: 4 per division)")
    for k, pretty in zip(names, demangle(names)):
        print(" ".join(f"{data[k][c]:6d}" for c in COLS) + "  " + pretty)
