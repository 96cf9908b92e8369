"""csrc/batch_arrays.h — the table of a handle's per-problem device arrays and the view that serves problems [b0, b0 + nb) by moving
every registered base pointer.  The header is pure host code: tests/c_abi/batch_arrays_table.cpp includes it alone, is compiled with
g++ and the address / undefined-behaviour sanitizers (an offset applied to a null pointer, or a read outside a buffer, ends the
program), and prints one line per check; the lines below are literals.

The buffers hold 9 problems, problem b's region filled with the byte b, at strides of 1, 4, 8, 12, 4099 and 2 * tasks * sizeof(int)
bytes; two more registered pointers are null.  "covers (b0, nb)": every buffer reads b0 at its first byte and b0 + nb - 1 at the last
byte of its nb-th region, and the null pointers are null."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHECKS = [
    "add",
    "single view (3, 4)", "single view restored",
    "edge (0, 9)", "edge (8, 1)", "edges restored",
    "nested level 1 (2, 6)", "nested level 2 (2 + 3, 3)", "nested level 3 (2 + 3 + 1, 2)",
    "nested level 3 closed", "nested level 2 closed", "nested level 1 closed",
    "sibling views (0, 5) then (5, 4)",
    "add rejects a duplicate slot", "add rejects a zero stride", "add rejects a negative stride", "add rejects a null slot",
    "rejections register nothing", "add rejects what a full table cannot hold",
]

# what a Float64 handle registers (csrc/handle.h: dalloc_batch, register_batch; csrc/capi_handle.cpp), in bytes per problem, for the
# program's constants: factor stride 1016, register-front scratch 364, work area 222, condensed stride 70, reduced order 31, band factor
# records 606 elements of 8 bytes; 5 tasks
STRIDES = [("d_L", 1016 * 8), ("d_gs", 364 * 8), ("d_scratch", 222 * 8), ("d_cbuf", 70 * 8), ("d_d2", 31 * 8), ("d_xpos", 4), ("d_xzer", 4),
           ("d_gcnt", 2 * 4), ("d_blk_ok", 4), ("d_sub_cnt", 2 * 5 * 4), ("d_Lband", 606 * 8)]


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("batch_arrays") / "batch_arrays_table")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "c_abi", "batch_arrays_table.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr)
    return r.stdout.splitlines()


def test_views_shift_nest_and_restore(lines):
    """Single view, both edges, three nested levels restored bit for bit in reverse order, sibling views, and what add() rejects."""
    assert [ln for ln in lines if not ln.startswith("stride ")] == [c + ": ok" for c in CHECKS]


def test_stride_table_of_a_handle(lines):
    """The registration list: these arrays, these strides, nothing else."""
    assert [ln for ln in lines if ln.startswith("stride ")] == [f"stride {name} {stride}" for name, stride in STRIDES]
