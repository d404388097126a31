"""The readings that several device calls share are stated once (csrc/se3quat.hpp for the three optimisers, csrc/map_gates.hpp for the
matchers), without a GPU.  (1) The copies are gone from the library's text.  (2) tools/se3quat_host.cpp, a program with its own main that
includes se3quat.hpp, is built with g++ under the address and undefined-behaviour sanitizers and run as it is; what it prints (hex floats)
is compared BIT FOR BIT with tests/pose_opt_ref.py.  Where the numpy definition uses `@` (se3_mul's translation, se3_map, the small-angle
branch of se3_exp), whose sum order numpy does not pin, the sums are restated here with scalar float64 operations in the header's written
order.  The trigonometric branch of se3_exp is not compared here (libm and numpy may differ in the last bit): the GPU tests of pose_opt
and local_ba cover it."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import pose_opt_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "a-low-texture-robust-hybrid-feature-based-visual-odometry_amd", "csrc")
HEADERS = ("se3quat.hpp", "map_gates.hpp")


def test_the_copies_are_gone_and_the_header_is_plain_cpp():
    ham = re.compile(r"(__popcll\([^;()]*\^[^;()]*\)\s*\+\s*){3}__popcll\(")              # three popcount(xor) terms and a plus
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith((".hip", ".hpp", ".inc")) or name in HEADERS:
            continue
        src = open(os.path.join(CSRC, name)).read()
        for pat in (r"\b(po|lb)_(quat_\w+|mat3|exp|mul|map)\(", r"\b(po|ls)_huber\(", r"bow_ham\(", r"pnp_xs32\("):
            assert not re.search(pat, src), (name, pat)
        for line in src.splitlines():
            assert not ham.search(line), (name, line.strip())
    for name in ("kf_search.hip", "fuse.hip", "local_points.hip", "local_lines.hip", "line_fuse.hip"):
        assert "logf(" not in open(os.path.join(CSRC, name)).read(), name
    gates = open(os.path.join(CSRC, "map_gates.hpp")).read()
    assert len([ln for ln in gates.splitlines() if ham.search(ln)]) == 1 and "int ham256(" in gates
    text = open(os.path.join(CSRC, "se3quat.hpp")).read()
    assert not re.search(r"#include\s*[<\"](hip|hvo_internal)", text)
    for name in ("pose_opt.hip", "local_ba.hip", "line_opt.hip"):
        assert '#include "se3quat.hpp"' in open(os.path.join(CSRC, name)).read(), name


# ---------------------------------------------------------------- the host program
def bits(v):
    return [struct.pack("<d", float(x)) for x in np.asarray(v, np.float64).ravel()]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("se3quat") / "se3quat_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover",
                           os.path.join(ROOT, "tools", "se3quat_host.cpp"), "-o", exe])

    def ask(requests):
        """requests: [(name, doubles)] -> the answers' doubles per printed line, in order"""
        text = "".join(name + "".join(" " + float(x).hex() for x in np.asarray(v, np.float64).ravel()) + "\n" for name, v in requests)
        out = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert out.returncode == 0, out.stderr.decode()[-2000:]
        lines = out.stdout.decode().split("\n")
        assert lines[-2] == "se3quat_host ok"
        return [[float.fromhex(t) if "x" in t or "n" in t else int(t) for t in ln.split()[1:]] for ln in lines[:-2]]
    return ask


def unit(q):
    q = np.asarray(q, np.float64)
    return q / np.sqrt(q @ q)


# one rotation per branch of Eigen::Quaterniond(Matrix3d): trace > 0, then the largest diagonal element at 0, 1 and 2
BRANCH_Q = [unit([0.9, 0.1, -0.2, 0.3]), unit([0.05, 0.95, 0.2, -0.1]), unit([-0.04, 0.15, 0.97, 0.1]), unit([0.03, -0.2, 0.1, 0.96])]


def test_quaternions_bit_for_bit(host):
    Rs = [ref.quat_to_R(q) for q in BRANCH_Q]
    branch = [0 if R[0, 0] + R[1, 1] + R[2, 2] > 0 else 1 + int(np.argmax(np.diag(R))) for R in Rs]
    assert branch == [0, 1, 2, 3]
    raw = [np.array([-0.7, 0.2, 0.5, -0.4]), np.array([0.3, -1.2, 0.8, 0.1])]           # w < 0, w > 0; neither is a unit quaternion
    got = host([("qfr", R) for R in Rs] + [("qn", q) for q in raw] + [("q2r", q) for q in BRANCH_Q])
    for R, g in zip(Rs, got[:4]):
        assert bits(g) == bits(ref.quat_from_R(R))
    for q, g in zip(raw, got[4:6]):
        assert bits(g) == bits(ref.quat_normalize(q.copy()))
    for q, g in zip(BRANCH_Q, got[6:]):
        assert bits(g) == bits(ref.quat_to_R(q))


def map_scalar(R, t, X):
    """se3_map's written order: ((R0 X0 + R1 X1) + R2 X2) + t"""
    return [((R[i][0] * X[0] + R[i][1] * X[1]) + R[i][2] * X[2]) + t[i] for i in range(3)]


def test_se3_mul_map_and_small_exp_bit_for_bit(host):
    f = lambda v: [float(x) for x in v]
    poses = [(BRANCH_Q[0], f([0.3, -0.2, 1.5])), (BRANCH_Q[2], f([-1.25, 0.75, 0.1])), (-BRANCH_Q[1], f([0.01, 2.0, -0.6]))]
    X = f([0.4, -0.7, 2.5])
    small = [f([3e-6, -2e-6, 1e-6, 0.01, -0.02, 0.03]), f([0, 0, 0, 0.5, 0.25, -1.0]), f([1e-9, 0, 0, 0, 0, 0]), f([0, 0, -1e-9, 0, 0, 0])]
    req = []
    for a in poses:
        for b in poses:
            req.append(("mul", np.concatenate([a[0], a[1], b[0], b[1]])))
    req += [("rt", np.concatenate([p[0], p[1]])) for p in poses]
    req += [("map", np.concatenate([ref.quat_to_R(p[0]).ravel(), p[1], X])) for p in poses]
    req += [("exp", u) for u in small]
    got = host(req)
    k = 0
    for a in poses:
        for b in poses:
            q = ref.quat_normalize(ref.quat_mul(a[0], b[0]))
            Ra = [f(r) for r in ref.quat_to_R(a[0])]
            t = [a[1][i] + ((Ra[i][0] * b[1][0] + Ra[i][1] * b[1][1]) + Ra[i][2] * b[1][2]) for i in range(3)]
            assert bits(got[k]) == bits(np.concatenate([q, t])); k += 1
    for p in poses:
        assert bits(got[k]) == bits(np.concatenate([ref.quat_to_R(p[0]).ravel(), p[1]])); k += 1
    for p in poses:
        assert bits(got[k]) == bits(map_scalar([f(r) for r in ref.quat_to_R(p[0])], p[1], X)); k += 1
    for u in small:
        assert np.sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]) < 0.00001
        Om = [0.0, -u[2], u[1], u[2], 0.0, -u[0], -u[1], u[0], 0.0]
        Om2 = [(Om[3 * i] * Om[j] + Om[3 * i + 1] * Om[3 + j]) + Om[3 * i + 2] * Om[6 + j] for i in range(3) for j in range(3)]
        R = [((1.0 if i % 4 == 0 else 0.0) + Om[i]) + Om2[i] for i in range(9)]
        q = ref.quat_normalize(ref.quat_from_R(np.array(R).reshape(3, 3)))
        t = [(R[3 * i] * u[3] + R[3 * i + 1] * u[4]) + R[3 * i + 2] * u[5] for i in range(3)]
        assert bits(got[k]) == bits(np.concatenate([q, t])); k += 1
    assert k == len(got)


def test_huber_bit_for_bit(host):
    delta = float(np.sqrt(5.991)); dsqr = delta * delta
    es = [0.25 * dsqr, dsqr, float(np.nextafter(dsqr, np.inf)), 40.0 * dsqr]             # below, at, just above, far above
    got = host([("hub", [e, delta]) for e in es])
    for e, g in zip(es, got):
        r0, r1, _ = ref.huber(e, delta, dsqr)
        assert bits(g) == bits([r0, r1])
    assert got[1] == [dsqr, 1.0] and got[2][1] < 1.0


def test_ldlt_bit_for_bit_and_the_two_pivot_rules(host):
    rng = np.random.RandomState(11)
    A = rng.standard_normal((6, 9))
    Hpd = A @ A.T + 0.5 * np.eye(6)
    Hneg = Hpd.copy(); Hneg[3, 3] = Hneg[3, 3] - 2.0 * Hpd[3, 3]                          # its fourth pivot is negative, none is zero
    b = rng.standard_normal(6)
    got = host([("ldl", np.concatenate([H.ravel(), b])) for H in (Hpd, Hneg)])
    for H, g, flags, want_ok in ((Hpd, got[0], got[1], True), (Hneg, got[2], got[3], False)):
        x, ok = ref.ldlt_solve(H, b)
        assert ok == want_ok and np.isfinite(x).all()
        assert bits(g) == bits(x)
        assert flags == [1 if ok else 0, 1]                                            # pose_opt's rule agrees; line_opt's accepts a negative pivot
