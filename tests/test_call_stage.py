"""The layout helper of the staging entry points (csrc/call_stage.hpp: StageCarver, StagePiece, stage_align, pose_split) without a GPU.
tools/call_stage_host.cpp, a program with its own main that includes the header, is built with g++ under the address and
undefined-behaviour sanitizers and run as it is: it asserts the alignment for 64 and 256, that an empty piece takes no space, the advance
per element size (1, 4, 8, 12, 28, 32 bytes), the row views up to the last element's last byte, the download view, that the host and the
device view of a piece differ by the difference of their bases, and fuse_run's layout against the offsets the hand arithmetic gave before
the helper existed.  The header stays host-only: no HIP header, no hipcc."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "a-low-texture-robust-hybrid-feature-based-visual-odometry_amd", "csrc")


def test_host_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "call_stage_host")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover",
                           os.path.join(ROOT, "tools", "call_stage_host.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    assert out.stdout.decode().strip() == "call_stage_host ok"


def test_header_is_host_only_and_the_sites_use_it():
    text = open(os.path.join(CSRC, "call_stage.hpp")).read()
    assert not re.search(r"#include\s*[<\"]hip|__device__|__global__|hipStream_t", text)
    for name in ("kf_search.hip", "fuse.hip", "new_points.hip", "pnp.hip", "bow.hip", "pose_opt.hip", "line_opt.hip"):
        src = open(os.path.join(CSRC, name)).read()
        assert "StageCarver C(" in src, name
    # the alignment helpers the sites used to carry are gone from the library's text
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".hpp", ".inc")) and name != "planes_tail.hip":              # (the plane tail's own al256 is a Frame-tail site)
            src = open(os.path.join(CSRC, name)).read()
            assert not re.search(r"\b(pal|al256|po_al|ls_al|sm_al)\(", src), name
