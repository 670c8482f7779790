"""CPU check of the slice rule of the co-scheduled hand-back list (zoe_amd/csrc/zsw_handback.hpp: handback_slice_rule,
handback_slices), no GPU: tests/models/handback_slices.cpp. The list the seed kernel leaves is scored by the first tier's shared
launch and by up to two slices on side streams; the one-thread kernel behind the seed kernel evaluates the same header function on
the device. A read no launch takes is never scored; a read two launches take is scored twice."""
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_exe = {}


def _build():
    if "handback_slices" not in _exe:
        exe = os.path.join(tempfile.mkdtemp(prefix="zsw_models_"), "handback_slices")
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-o", exe, os.path.join(ROOT, "tests", "models", "handback_slices.cpp")], check=True)
        _exe["handback_slices"] = exe
    return _exe["handback_slices"]


def test_the_three_ranges_partition_the_list_and_exactly_one_launch_takes_each_read():
    """Both switches, the call on its own stream or not, classes on either side of HANDBACK_SLICE_MIN_CLASS; every n0 in
    0 .. 3 x (head + tail + one round), which passes every threshold of the rule; and hand-made rules with a head or a tail alone."""
    out = subprocess.run([_build(), "sweep"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    checks, violations = (int(v) for v in re.fullmatch(r"handback_slices sweep: (\d+) checks, (\d+) violations", lines[-1]).groups())
    assert checks >= 6 * 8 * 3 * 98304
    assert violations == len(lines) - 1 == 0, lines[:10]


def test_slices_are_planned_only_where_the_full_pass_is_coscheduled_on_the_callers_stream():
    out = subprocess.run([_build(), "decide"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    pat = re.compile(r"DECIDE (\d) (\d) (\d) (\d+) (\d) (\d) (\d) (\d) (\d) (\d) (\d) (\d) (\d+) -> (\d+) (\d+)")
    rows = [tuple(int(v) for v in pat.fullmatch(ln).groups()) for ln in out.stdout.splitlines()]
    assert len(rows) == len(set(r[:-2] for r in rows)) == 3 * 2 * 512 * 6
    for r in rows:
        mode, two, diag, g, mins, chunks, skip, disabled, cosched, own, no_slices, tiny, cls, head, tail = r
        assert cosched == int(mode == 0 and two and diag and g == 4 and not (mins or chunks or skip or disabled)), r
        if not cosched or not own or no_slices:
            assert (head, tail) == (0, 0), r
        elif tiny:
            assert (head, tail) == (128, 128), r  # the sizes the header names for ZSW_DEBUG_SEED_TINY_SLICES
        elif cls < 2097152:
            assert (head, tail) == (0, 0), r
        else:
            assert 0 < tail <= 32768 and head in (0, 32768), r
    assert any(r[-1] for r in rows)


def test_the_tail_slice_leaves_registers_for_the_second_tier():
    """One wavefront of seed_band_kernel<48,2,0> and one of the remainder launch must fit beside the tail's resident wavefronts in
    the 512 VGPRs of a SIMD, and the tail's bound is those wavefronts on 1,024 SIMDs at 32 reads each."""
    out = subprocess.run([_build(), "budget"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    waves, v_tail, v_band, v_rem, per_simd, tail_reads, tail_g = (int(v) for v in re.fullmatch(r"BUDGET (\d+) (\d+) (\d+) (\d+) (\d+) (\d+) (\d+)", out.stdout.strip()).groups())
    assert per_simd == 512 and waves >= 1
    assert (tail_g, v_tail) in ((4, 144), (8, 96))  # score_kernel_v2<4,38,0> / <8,19,0>
    assert waves * v_tail + v_band + v_rem <= per_simd
    assert 0 < tail_reads <= waves * 1024 * (128 // tail_g)
