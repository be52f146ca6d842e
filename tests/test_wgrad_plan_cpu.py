"""The launch plan of the 1x1 weight-gradient / Gram kernels (efficientat_amd/csrc/wgrad_plan.h) without a GPU: the five host
helpers against a table of the training steps' launches, and the plan's structure over a grid of requests by a stand-alone
checker (tests/wgrad_plan_check.cpp) built with AddressSanitizer and UBSan."""
import os
import shutil
import subprocess

import pytest

from efficientat_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.lib()


# Which kernel each 1x1 weight-gradient / Gram launch of one training step runs on - mn10 at batch 256, mn40 with bf16 storage
# and dymn20 at batch 128 (128 mels x 1000 frames) - and how many workspace copies give every block its own.  Recorded from the
# library as it stood BEFORE the plan moved into wgrad_plan.h (the calls of one eager step, the helpers asked per call); a
# changed row is a changed launch plan, to be measured like one.
#   entry: the eat_pw_conv_* / eat_gram_centered entry point; mode 0 = bf16x3, 2 = plain bf16; options: same = dz is x, scale = an
#   SE scale multiplies x, tf = BatchNorm + activation of x on load
#   kernel: narrow MxN [gram] = pw_wgrad_x3_narrow_kernel<M, N>, x3 = pw_wgrad_x3_kernel (128 x 128 tiles), wide = pw_wgrad_wide_kernel
#   (dymn20's batch-1 rows are the weight gradients of its context / coefficient GEMMs, batch folded into S)
# (model, entry, B, Co, Ci, S, mode, options) -> (kernel, slots)
FP32_STORAGE = [
    ('mn10',      'gram_centered', 256,   16,  16, 32000, 0, 'same',     'narrow 1x1 gram', 1024),
    ('mn10',      'gram_centered', 256,   24,  24,  8000, 0, 'same',     'narrow 2x2 gram', 1016),
    ('mn10',      'gram_centered', 256,   40,  40,  2000, 0, 'same',     'narrow 3x3 gram', 1008),
    ('mn10',      'gram_centered', 256,   80,  80,   504, 0, 'same',     'wide',             256),
    ('mn10',      'gram_centered', 256,  112, 112,   504, 0, 'same',     'wide',             256),
    ('mn10',      'gram_centered', 256,  160, 160,   128, 0, 'same',     'wide',              64),
    ('mn10',      'wgrad_ws',      256,  960, 160,   128, 0, '-',        'wide',              64),
    ('mn10',      'wgrad_ws',      256,  160, 960,   128, 0, 'scale',    'wide',              64),
    ('mn10',      'wgrad_ws',      256,  160, 672,   128, 0, 'scale',    'wide',              64),
    ('mn10',      'wgrad_ws',      256,  672, 112,   504, 0, '-',        'wide',              84),
    ('mn10',      'wgrad_ws',      256,  112, 672,   504, 0, 'scale',    'wide',              84),
    ('mn10',      'wgrad_ws',      256,  112, 480,   504, 0, 'scale',    'wide',             128),
    ('mn10',      'wgrad_ws',      256,  480,  80,   504, 0, '-',        'wide',             128),
    ('mn10',      'wgrad_tf',      256,   80, 184,   504, 0, 'tf',       'x3',               256),
    ('mn10',      'wgrad_ws',      256,  184,  80,   504, 0, '-',        'wide',             256),
    ('mn10',      'wgrad_tf',      256,   80, 200,   504, 0, 'tf',       'x3',               256),
    ('mn10',      'wgrad_ws',      256,  200,  80,   504, 0, '-',        'wide',             256),
    ('mn10',      'wgrad_tf',      256,   80, 240,   504, 0, 'tf',       'x3',               256),
    ('mn10',      'wgrad_ws',      256,  240,  40,  2000, 0, '-',        'wide',             256),
    ('mn10',      'wgrad_tf',      256,   40, 120,  2000, 0, 'scale tf', 'narrow 3x3',       256),
    ('mn10',      'wgrad_ws',      256,  120,  40,  2000, 0, '-',        'wide',             256),
    ('mn10',      'wgrad_tf',      256,   40,  72,  2000, 0, 'scale tf', 'narrow 3x3',       504),
    ('mn10',      'wgrad',         256,   72,  24,  8000, 0, '-',        'narrow 5x2',      1016),
    ('mn10',      'wgrad_tf',      256,   24,  72,  8000, 0, 'tf',       'narrow 2x5',      1016),
    ('mn10',      'wgrad_tf',      256,   24,  64,  8000, 0, 'tf',       'narrow 2x2',       512),
    ('mn10',      'wgrad_ws',      256,   64,  16, 32000, 0, '-',        'narrow 4x1',      1024),
    ('mn10',      'wgrad_tf',      256,   16,  16, 32000, 0, 'tf',       'narrow 1x1',      1024),
    ('mn40_bf16', 'gram_centered', 128,   64,  64, 32000, 2, 'same',     'narrow 4x4 gram', 1024),
    ('mn40_bf16', 'gram_centered', 128,   96,  96,  8000, 2, 'same',     'wide',             256),
    ('mn40_bf16', 'gram_centered', 128,  160, 160,  2000, 2, 'same',     'wide',             252),
    ('mn40_bf16', 'gram_centered', 128,  320, 320,   504, 2, 'same',     'x3',                56),
    ('mn40_bf16', 'gram_centered', 128,  448, 448,   504, 2, 'same',     'x3',                32),
    ('mn40_bf16', 'gram_centered', 128,  640, 640,   128, 2, 'same',     'x3',                20),
    ('mn40_bf16', 'wgrad_ws',      128, 3840, 640,   128, 2, '-',        'wide',               4),
    ('dymn20',    'wgrad_ws',      128, 1920, 320,   128, 0, '-',        'wide',              16),
    ('dymn20',    'wgrad_ws',        1, 1920, 256,  4096, 0, '-',        'wide',               8),
    ('dymn20',    'wgrad_ws',        1, 1920, 256,   512, 0, '-',        'wide',               1),
    ('dymn20',    'wgrad_ws',        1,  256, 320,  4608, 0, '-',        'wide',               9),
    ('dymn20',    'wgrad_ws',        1, 1344, 256,  4096, 0, '-',        'wide',               8),
    ('dymn20',    'wgrad_ws',        1, 1344, 256,   512, 0, '-',        'wide',               1),
    ('dymn20',    'wgrad_ws',        1,  256, 224,  9088, 0, '-',        'wide',              17),
    ('dymn20',    'wgrad_ws',        1, 1344, 256,  8064, 0, '-',        'wide',              15),
    ('dymn20',    'wgrad_ws',        1, 1344, 256,  1024, 0, '-',        'wide',               2),
    ('dymn20',    'wgrad_ws',        1,  960, 240,  8064, 0, '-',        'wide',              15),
    ('dymn20',    'wgrad_ws',        1,  960, 240,  1024, 0, '-',        'wide',               2),
    ('dymn20',    'wgrad_ws',        1,  240, 160,  9088, 0, '-',        'wide',              17),
    ('dymn20',    'wgrad_ws',        1,  368,  96,  8064, 0, '-',        'wide',              15),
    ('dymn20',    'wgrad_ws',        1,  368,  96,  1024, 0, '-',        'wide',               2),
    ('dymn20',    'wgrad_ws',        1,   96, 160,  9088, 0, '-',        'wide',              17),
    ('dymn20',    'wgrad_ws',        1,  400, 104,  8064, 0, '-',        'wide',              15),
    ('dymn20',    'wgrad_ws',        1,  400, 104,  1024, 0, '-',        'wide',               2),
    ('dymn20',    'wgrad_ws',        1,  104, 160,  9088, 0, '-',        'wide',              17),
    ('dymn20',    'wgrad_ws',        1,  480, 120,  8064, 0, '-',        'wide',              15),
    ('dymn20',    'wgrad_ws',        1,  480, 120,  1024, 0, '-',        'wide',               2),
    ('dymn20',    'wgrad_ws',        1,  120,  80, 18048, 0, '-',        'wide',              34),
    ('dymn20',    'wgrad_ws',        1,  240,  64, 16000, 0, '-',        'wide',              30),
    ('dymn20',    'wgrad_ws',        1,  240,  64,  2048, 0, '-',        'wide',               4),
    ('dymn20',    'wgrad',           1,   64,  80, 18048, 0, '-',        'x3',                34),
    ('dymn20',    'wgrad_ws',        1,  144,  64, 16000, 0, '-',        'wide',              30),
    ('dymn20',    'wgrad_ws',        1,  144,  64,  2048, 0, '-',        'wide',               4),
    ('dymn20',    'wgrad_ws',        1,   64,  48, 36096, 0, '-',        'x3',                67),
    ('dymn20',    'wgrad_ws',        1,  144,  64, 32000, 0, '-',        'wide',              59),
    ('dymn20',    'wgrad_ws',        1,  144,  64,  4096, 0, '-',        'wide',               8),
    ('dymn20',    'wgrad_ws',        1,  128,  64, 32000, 0, '-',        'wide',              59),
    ('dymn20',    'wgrad_ws',        1,  128,  64,  4096, 0, '-',        'wide',               8),
    ('dymn20',    'wgrad_ws',        1,   64,  32, 72192, 0, '-',        'x3',               141),
    ('dymn20',    'wgrad_ws',        1,   32,  64, 64000, 0, '-',        'x3',               125),
    ('dymn20',    'wgrad_ws',        1,   32,  64,  8192, 0, '-',        'x3',                16),
]
# eat_pw_conv_wgrad_b16 (always the wide-tile kernel): (model, B, Co, Ci, S, x_b16) -> slots
BF16_STORAGE = [
    ('mn40_bf16', 128,  640, 3840,   128, 1,   4),
    ('mn40_bf16', 128, 3840,  640,   128, 0,   4),
    ('mn40_bf16', 128,  640, 2688,   128, 1,   5),
    ('mn40_bf16', 128, 2688,  448,   504, 0,   7),
    ('mn40_bf16', 128,  448, 2688,   504, 1,   7),
    ('mn40_bf16', 128,  448, 1920,   504, 1,  10),
    ('mn40_bf16', 128, 1920,  320,   504, 0,  16),
    ('mn40_bf16', 128,  320,  736,   504, 1,  42),
    ('mn40_bf16', 128,  736,  320,   504, 0,  42),
    ('mn40_bf16', 128,  320,  800,   504, 1,  32),
    ('mn40_bf16', 128,  800,  320,   504, 0,  32),
    ('mn40_bf16', 128,  320,  960,   504, 1,  32),
    ('mn40_bf16', 128,  960,  160,  2000, 0,  64),
    ('mn40_bf16', 128,  160,  480,  2000, 1, 128),
    ('mn40_bf16', 128,  480,  160,  2000, 0, 128),
    ('mn40_bf16', 128,  160,  288,  2000, 1, 128),
    ('mn40_bf16', 128,  288,   96,  8000, 0, 128),
    ('mn40_bf16', 128,   96,  288,  8000, 1, 128),
    ('mn40_bf16', 128,   96,  256,  8000, 1, 256),
    ('mn40_bf16', 128,  256,   64, 32000, 0, 256),
    ('mn40_bf16', 128,   64,   64, 32000, 1, 256),
]
# eat_pw_conv_dyn_wgrad_b16 with both operands fp32 (x_b16 = 2), the per-sample gradients of dymn20's dynamic convs:
# (model, B, Co, Ci, S, x_b16) -> (k-slices per sample, eat_pw_dyn_wgrad_accumulates(Co, Ci, S) of the streaming alternative)
PER_SAMPLE = [
    ('dymn20', 128,  320, 1920,   128, 2, 1, 0),
    ('dymn20', 128, 1920,  320,   128, 2, 1, 0),
    ('dymn20', 128,  320, 1344,   128, 2, 1, 0),
    ('dymn20', 128, 1344,  224,   504, 2, 1, 0),
    ('dymn20', 128,  224, 1344,   504, 2, 1, 0),
    ('dymn20', 128,  224,  960,   504, 2, 1, 0),
    ('dymn20', 128,  960,  160,   504, 2, 2, 0),
    ('dymn20', 128,  160,  368,   504, 2, 2, 0),
    ('dymn20', 128,  368,  160,   504, 2, 2, 0),
    ('dymn20', 128,  160,  400,   504, 2, 2, 0),
    ('dymn20', 128,  400,  160,   504, 2, 2, 0),
    ('dymn20', 128,  160,  480,   504, 2, 2, 0),
    ('dymn20', 128,  480,   80,  2000, 2, 4, 0),
    ('dymn20', 128,   80,  240,  2000, 2, 4, 0),
    ('dymn20', 128,  240,   80,  2000, 2, 4, 0),
    ('dymn20', 128,   80,  144,  2000, 2, 4, 0),
    ('dymn20', 128,  144,   48,  8000, 2, 8, 1),
    ('dymn20', 128,   48,  144,  8000, 2, 8, 1),
    ('dymn20', 128,   48,  128,  8000, 2, 8, 1),
    ('dymn20', 128,  128,   32, 32000, 2, 8, 1),
    ('dymn20', 128,   32,   32, 32000, 2, 8, 1),
]


def _kind(kernel):
    """eat_pw_wgrad_kernel_kind's encoding of a table entry: kind + 10 * (1000 mtb + 10 ntb + gram)."""
    if kernel in ("x3", "fp32", "wide"):
        return {"x3": 1, "fp32": 2, "wide": 3}[kernel]
    _, pair, *gram = kernel.split()
    m, n = pair.split("x")
    return 10 * (1000 * int(m) + 10 * int(n) + (1 if gram else 0))


@pytest.mark.parametrize("row", FP32_STORAGE, ids=lambda r: f"{r[0]}-{r[1]}-{r[3]}x{r[4]}x{r[5]}-{r[7].replace(' ', '+')}")
def test_kernel_kind_and_slots_of_the_training_steps(lib, row):
    model, entry, B, Co, Ci, S, mode, options, kernel, slots = row
    same, scale, tf = ("same" in options.split(), "scale" in options.split(), "tf" in options.split())
    assert lib.eat_pw_wgrad_kernel_kind(B, Co, Ci, S, mode, int(same), int(scale), int(tf)) == _kind(kernel)
    assert lib.eat_pw_wgrad_slots(B, Co, Ci, S, mode, int(same)) == slots


def test_exact_fp32_and_unaligned_shapes_leave_the_bf16_kernels(lib):
    """mode 1 (and S % 4 != 0) is the exact-fp32 kernel whatever the shape; a wide-tile shape whose rows of dW are not 16-byte
    aligned (Ci % 4 != 0) answers with the plan the launch falls back to."""
    for model, entry, B, Co, Ci, S, mode, options, kernel, slots in FP32_STORAGE:
        same = int("same" in options.split())
        assert lib.eat_pw_wgrad_kernel_kind(B, Co, Ci, S, 1, same, 0, 0) == 2
        assert lib.eat_pw_wgrad_kernel_kind(B, Co, Ci, S + 2, mode, same, 0, 0) == 2
    assert lib.eat_pw_wgrad_kernel_kind(2, 96, 64, 64, 0, 0, 0, 0) == 3
    assert lib.eat_pw_wgrad_kernel_kind(2, 96, 66, 64, 0, 0, 0, 0) == 1


@pytest.mark.parametrize("row", BF16_STORAGE, ids=lambda r: f"{r[0]}-{r[2]}x{r[3]}x{r[4]}-{r[5]}")
def test_bf16_storage_slots_of_the_mn40_step(lib, row):
    model, B, Co, Ci, S, x_b16, slots = row
    assert lib.eat_pw_wgrad_b16_slots(B, Co, Ci, S, x_b16) == slots


@pytest.mark.parametrize("row", PER_SAMPLE, ids=lambda r: f"{r[0]}-{r[2]}x{r[3]}x{r[4]}")
def test_per_sample_slices_of_the_dymn20_step(lib, row):
    model, B, Co, Ci, S, x_b16, slices, accumulates = row
    assert lib.eat_pw_dyn_wgrad_b16_slices(B, Co, Ci, S, x_b16) == slices
    assert lib.eat_pw_dyn_wgrad_accumulates(Co, Ci, S) == accumulates
    assert lib.eat_pw_dyn_wgrad_b16_slices(B, Co, Ci + 2, S, x_b16) == 0          # Ci % 4 != 0: not on the wide-tile kernel


def test_plan_structure_over_a_grid_under_sanitizers(tmp_path):
    """tests/wgrad_plan_check.cpp: every plan of the grid is a launchable cover of its problem (no empty block, an existing
    streaming instance, row groups and wide tiles that cover Co x Ci within the kernels' limits, the LDS budget, per-sample
    slices that own a unit each).  A program of its own, built by the host compiler with -fsanitize=address,undefined."""
    # the sanitizer runtimes are linked statically: the program then runs the same whatever the environment preloads
    gxx = shutil.which("g++")
    cmd = [gxx, "-static-libasan", "-static-libubsan"] if gxx else [shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++", "-static-libsan"]
    exe = str(tmp_path / "wgrad_plan_check")
    subprocess.run(cmd + ["-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                          "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "efficientat_amd", "csrc"),
                          os.path.join(ROOT, "tests", "wgrad_plan_check.cpp"), "-o", exe], check=True)
    env = {k: v for k, v in os.environ.items() if k != "EAT_WGRAD_FP32"}      # (the debug override would plan every request as fp32)
    r = subprocess.run([exe], env=env, capture_output=True, text=True)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert " 0 violations" in r.stdout
