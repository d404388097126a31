#!/usr/bin/env python3
"""Per-kernel register, spill, scratch and LDS figures of HIP sources, from the compiler's own remarks.

    tools/kernel_resources.py csrc/orb_level.hip csrc/peac.hip ...

Each file is compiled for the device only, with the CXXFLAGS of the library's Makefile plus
-Rpass-analysis=kernel-resource-usage; nothing is linked or kept.  "alloc" is the VGPR count rounded up to the
allocation granule of 8 (gfx950: 512 registers per lane per SIMD), which is what decides who fits beside whom.
Only the remarks are read, never the assembly."""
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "a-low-texture-robust-hybrid-feature-based-visual-odometry_amd", "csrc")
GRANULE = 8
FILE_PER_SIMD = 512

_FIELDS = {
    "TotalSGPRs": "sgprs", "SGPRs": "sgprs", "VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize [bytes/lane]": "scratch",
    "Occupancy [waves/SIMD]": "occupancy", "SGPRs Spill": "sgpr_spills", "VGPRs Spill": "vgpr_spills", "LDS Size [bytes/block]": "lds",
}


def _make_var(name, default):
    """NAME ?= value of the library's Makefile (one line, $(ARCH) expanded by the caller)"""
    with open(os.path.join(CSRC, "Makefile")) as f:
        for line in f:
            m = re.match(r"\s*%s\s*\??=\s*(.*)$" % re.escape(name), line)
            if m:
                return m.group(1).strip()
    return default


def hipcc():
    return os.environ.get("HIPCC") or (_make_var("HIPCC", "") if os.path.exists(_make_var("HIPCC", "")) else None) or shutil.which("hipcc")


def cxxflags():
    arch = os.environ.get("ARCH") or _make_var("ARCH", "gfx950")
    return _make_var("CXXFLAGS", "-O3").replace("$(ARCH)", arch).split()


def demangle(names):
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not filt or not names:
        return list(names)
    out = subprocess.run([filt], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout
    return out.splitlines()


def short_name(dem):
    """'void k_orb_level<4>(LevelArgs)' -> 'k_orb_level<4>'"""
    s = re.sub(r"^void\s+", "", dem)
    depth = 0
    for i, ch in enumerate(s):
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            return s[:i]
    return s


def resources(path, extra=()):
    """{kernel: {vgprs, alloc, sgprs, sgpr_spills, vgpr_spills, scratch, lds, occupancy}} of one .hip file"""
    cc = hipcc()
    if not cc:
        raise RuntimeError("hipcc not found")
    path = os.path.abspath(path)
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [cc] + cxxflags() + list(extra) + ["--offload-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", path, "-o", os.path.join(tmp, "dev.o")]
        r = subprocess.run(cmd, cwd=os.path.dirname(path), capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("%s failed:\n%s" % (" ".join(cmd), r.stderr[-4000:]))
    recs, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?):\s+(\S+)\s+\[-Rpass-analysis=kernel-resource-usage\]", line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            cur = {"mangled": val}
            recs.append(cur)
        elif cur is not None and key in _FIELDS:
            cur[_FIELDS[key]] = int(val)
    out = {}
    for rec, dem in zip(recs, demangle([r_["mangled"] for r_ in recs])):
        if "vgprs" not in rec:
            continue
        rec["alloc"] = (rec["vgprs"] + rec.get("agprs", 0) + GRANULE - 1) // GRANULE * GRANULE
        out[short_name(dem)] = rec
    return out


def main(argv):
    as_json = "--json" in argv
    files = [a for a in argv if not a.startswith("--")]
    if not files:
        print(__doc__)
        return 2
    allk = {}
    for f in files:
        res = resources(f)
        allk[os.path.basename(f)] = res
        if as_json:
            continue
        print("%s" % os.path.basename(f))
        print("  %-44s %5s %5s %5s %6s %6s %7s %7s" % ("kernel", "VGPR", "alloc", "SGPR", "s-spil", "v-spil", "scratch", "LDS"))
        for k in sorted(res):
            r = res[k]
            print("  %-44s %5d %5d %5d %6d %6d %7d %7d" % (k[:44], r["vgprs"], r["alloc"], r.get("sgprs", 0), r.get("sgpr_spills", 0), r.get("vgpr_spills", 0), r.get("scratch", 0), r.get("lds", 0)))
    if as_json:
        print(json.dumps(allk, indent=1, sort_keys=True))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
