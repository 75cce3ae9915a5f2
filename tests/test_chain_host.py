"""The modified-DH chain of csrc/chain.h on the CPU (tests/chain_host/chain_host.cpp, a plain C++ program that includes the header alone)
against two references that share no code with it: oracle.success_oracle.link_box_poses (4 x 4 NumPy products from franka.DH_A_D_ALPHA and
franka.static_frames) and tests/ik_inputs.fk with the reference's end-effector tool (evaluation._dh, evaluation.EE_STATIC_DH).

Gates, derived and not measured: the chain is at most ten 3 x 4 products whose entries stay below 2 in magnitude, every entry a sum of
four terms, so a rounding error of about 10 * 4 * 2 * 2^-53 ~ 1e-14 absolute; the f64 gate is 1e-13.  The f32 leg, fed the same f64 sines
and cosines rounded to f32, is held to the f64 leg at 5e-5, the same bound with 2^-24.  A wrong index, sign or frame moves a link by
millimetres."""
import os
import subprocess

import numpy as np
import pytest

from edmp_amd import franka
from oracle import success_oracle as SO
from tests import ik_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64_GATE, F32_GATE = 1e-13, 5e-5


def configurations() -> np.ndarray:
    """(67, 7): 64 drawn inside the limits with RandomState(0), the all-zero configuration, both limit vectors"""
    lo, hi = franka.joint_limits()
    return np.concatenate([np.random.RandomState(0).uniform(lo, hi, (64, 7)), np.zeros((1, 7)), lo[None], hi[None]])


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """the program's output, parsed: tables {name: array}, frames [configuration][type][(what, k)] = (3, 4) array"""
    exe = os.path.join(ROOT, "tests", "chain_host", "chain_host")
    if not os.path.exists(exe):  # normally prebuilt by __graft_entry__.build(); compile here otherwise (plain g++)
        exe = str(tmp_path_factory.mktemp("chain_host") / "chain_host")
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-I" + os.path.join(ROOT, "edmp_amd", "csrc"),
                        os.path.join(ROOT, "tests", "chain_host", "chain_host.cpp"), "-o", exe], check=True)
    numbers = list(franka.static_frames().astype(np.float64).ravel()) + list(configurations().ravel())
    out = subprocess.run([exe], input=" ".join(float(v).hex() for v in numbers), capture_output=True, text=True, check=True).stdout
    tables, frames = {}, []
    for line in out.splitlines():
        w = line.split()
        if w[0] in ("qlo", "qhi", "dh"):
            tables[w[0]] = np.array([float.fromhex(v) for v in w[1:]])
        elif w[0] == "q":
            assert int(w[1]) == len(frames)
            frames.append({"f64": {}, "f32": {}})
        else:
            frames[-1][w[0]][(w[1], int(w[2]))] = np.array([float.fromhex(v) for v in w[3:]]).reshape(3, 4)
    assert len(frames) == len(configurations())
    for f in frames:
        for t in ("f64", "f32"):
            assert sorted(f[t]) == sorted([("joint", j) for j in range(7)] + [("link", l) for l in range(9)] + [("ee", 0)])
    return tables, frames


def test_the_header_tables_are_frankas_bit_for_bit(run):
    tables, _ = run
    lo, hi = franka.joint_limits()
    assert tables["qlo"].tobytes() == lo.tobytes() and tables["qhi"].tobytes() == hi.tobytes()
    assert tables["dh"].tobytes() == np.ascontiguousarray(franka.dh_table_f64()).tobytes()


def test_f64_link_boxes_against_the_success_oracle(run):
    _, frames = run
    worst = 0.0
    for q, f in zip(configurations(), frames):
        for l, (R, c) in enumerate(SO.link_box_poses(q)):
            worst = max(worst, np.abs(f["f64"][("link", l)] - np.concatenate([R, c[:, None]], axis=1)).max())
    print(f"f64 link boxes vs success_oracle.link_box_poses: max |diff| = {worst:.3e} (gate {F64_GATE:g})")
    assert worst <= F64_GATE


def test_f64_joint7_and_end_effector_against_the_ik_reference_fk(run):
    _, frames = run
    worst = 0.0
    for q, f in zip(configurations(), frames):
        worst = max(worst, np.abs(f["f64"][("ee", 0)] - ik_inputs.fk(q)[:3]).max())  # tool None: the reference's end-effector rows
        worst = max(worst, np.abs(f["f64"][("joint", 6)] - ik_inputs.fk(q, np.eye(4)[:3])[:3]).max())
    print(f"f64 joint 7 / end effector vs ik_inputs.fk: max |diff| = {worst:.3e} (gate {F64_GATE:g})")
    assert worst <= F64_GATE


def test_f32_chain_follows_the_f64_chain(run):
    _, frames = run
    worst = max(np.abs(f["f32"][k] - f["f64"][k]).max() for f in frames for k in f["f64"])
    print(f"f32 chain vs f64 chain, all 17 frames: max |diff| = {worst:.3e} (gate {F32_GATE:g})")
    assert worst <= F32_GATE
