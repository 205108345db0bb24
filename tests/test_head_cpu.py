"""What the calls of the two controllers share on the host (csrc/host_head.h) without a GPU: the parameter count
and the common shape check through a stand-alone C++ driver (tests/head_driver.cpp), plain and under the address and
undefined-behaviour sanitizers, against the Python layer's counts and the message strings pic_policy_* and pic_actor_* have
always returned."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "optimal-control-1d-electrostatic-plasma_amd", "csrc")
WIDTHS = (0, 1, 2, 255, 256, 257)


def _build(tmp, name, extra):
    out = str(tmp / name)
    args = ["-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC] + extra + [os.path.join(ROOT, "tests", "head_driver.cpp"), "-o", out]
    cxx = shutil.which("c++")
    if cxx:
        cmd = [cxx] + args
    else:
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        if not os.path.exists(hipcc):
            pytest.skip("no host C++ compiler (c++ or hipcc) to build tests/head_driver.cpp with")
        cmd = [hipcc, "-x", "c++"] + args
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr

    def run(rows):
        p = subprocess.run([out], input="".join(" ".join(map(str, r)) + "\n" for r in rows), capture_output=True, text=True)
        assert p.returncode == 0 and not p.stderr, p.stderr
        res = p.stdout.splitlines()
        assert len(res) == len(rows)
        return res
    return run


def _rows():
    """(max_layers, n_layers, w0 .. w7, layernorm, mem_kind, activation, squash, per_env, has_params): for both controllers
    every n_layers in 0..7 with widths that are all valid, all drawn from WIDTHS, and valid but for one bad width at every
    place; then, on a valid shape, every single bad flag and every pair of faults."""
    rng = np.random.default_rng(7)
    ok = (0, 0, 0, 0, 1)                            # mem_kind, activation, squash, per_env, has_params
    rows = []
    for max_layers, n, ln in itertools.product((4, 6), range(8), (0, 1)):
        good = [int(w) for w in rng.choice((1, 2, 255, 256), 8)]
        rows.append((max_layers, n, *good, ln, *ok))
        rows.append((max_layers, n, *(int(w) for w in rng.choice(WIDTHS, 8)), ln, *ok))
        for at, w in zip(range(8), itertools.cycle((0, 257))):
            rows.append((max_layers, n, *good[:at], w, *good[at + 1:], ln, *ok))
    bad = {0: (2, -1), 1: (2, -1), 2: (2, -1), 3: (2, -1), 4: (0,)}      # per flag: its bad values
    for max_layers in (4, 6):
        shape = (max_layers, 2, 4, 256, 2, 0, 0, 0, 0, 0, 1)
        for i, values in bad.items():
            rows += [shape + ok[:i] + (v,) + ok[i + 1:] for v in values]
        for (i, vi), (j, vj) in itertools.combinations([(i, v[0]) for i, v in bad.items()], 2):
            flags = list(ok)
            flags[i], flags[j] = vi, vj
            rows.append(shape + tuple(flags))
            rows.append((max_layers, 0) + shape[2:] + tuple(flags))             # ... and with n_layers = 0 on top
            rows.append(shape[:3] + (257,) + shape[4:] + tuple(flags))          # ... and with a bad width on top
    return rows


def _message(max_layers, n, widths, mem_kind, activation, squash, per_env, has_params):
    """policy_bad_args' and actor_bad_args' checks of the fields both structs have, in their order, with their strings."""
    if mem_kind not in (0, 1):
        return "bad mem_kind"
    if not 1 <= n <= max_layers:
        return {4: "n_layers must be 1..4", 6: "n_layers must be 1..6"}[max_layers]
    if any(not 1 <= w <= 256 for w in widths[:n + 1]):
        return "every width must be 1..256"
    if activation not in (0, 1):
        return "activation must be PIC_ACT_TANH or PIC_ACT_RELU"
    if squash not in (0, 1):
        return "squash must be 0 or 1"
    if per_env not in (0, 1):
        return "per_env must be 0 or 1"
    return "ok" if has_params else "null params"


def test_param_count_and_shape_check_plain_and_sanitized(tmp_path):
    from ocplasma_amd.control.actor import head_param_count
    from ocplasma_amd.control.policy import param_count
    plain = _build(tmp_path, "head_driver", [])
    sanitized = _build(tmp_path, "head_driver_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    # pinned rows: a 3-layer policy [4, 8, 8, 2]; the same widths as a head with LayerNorms; two faults at once
    assert plain([(4, 3, 4, 8, 8, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1), (6, 3, 4, 8, 8, 2, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1),
                  (4, 5, 4, 8, 8, 2, 1, 1, 0, 0, 0, 2, 0, 0, 0, 1), (6, 5, 4, 8, 8, 2, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0)]) == [
        "P=130 ok", "P=162 ok", "P=135 bad mem_kind", "P=135 null params"]
    rows = _rows()
    assert 300 <= len(rows) <= 1000
    for run in (plain, sanitized):
        for row, got in zip(rows, run(rows)):
            max_layers, n, widths, ln, flags = row[0], row[1], list(row[2:10]), row[10], row[11:]
            P = head_param_count(widths[:n + 1], bool(ln))
            if not ln:
                assert P == param_count(widths[:n + 1])
            assert got == f"P={P} {_message(max_layers, n, widths, *flags)}", row
    # every message of the shared check is reached, for both controllers
    seen = {(r[0], _message(r[0], r[1], list(r[2:10]), *r[11:])) for r in rows}
    for max_layers in (4, 6):
        assert {m for k, m in seen if k == max_layers} == {
            "ok", "bad mem_kind", f"n_layers must be 1..{max_layers}", "every width must be 1..256",
            "activation must be PIC_ACT_TANH or PIC_ACT_RELU", "squash must be 0 or 1", "per_env must be 0 or 1", "null params"}
