"""The route of the forward 1x1 convolutions (efficientat_amd/csrc/pw_fwd_plan.h) without a GPU: the stand-alone checker
(tests/pw_fwd_plan_check.cpp: the table of the models' and the edge cases' launches, the rules of check(), the plan's structure
over a grid) built with AddressSanitizer and UBSan, and the entry points' own refusals against the library."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from efficientat_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.lib()


def test_route_table_rules_and_structure_under_sanitizers(tmp_path):
    """A program of its own, built by the host compiler with -fsanitize=address,undefined: every recorded launch still gets its
    kernel instance, grid and LDS size; every shared rule refuses; every plan of the grid is a launchable cover of its problem."""
    # the sanitizer runtimes are linked statically: the program then runs the same whatever the environment preloads
    gxx = shutil.which("g++")
    cmd = [gxx, "-static-libasan", "-static-libubsan"] if gxx else [shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++", "-static-libsan"]
    exe = str(tmp_path / "pw_fwd_plan_check")
    subprocess.run(cmd + ["-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                          "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "efficientat_amd", "csrc"),
                          os.path.join(ROOT, "tests", "pw_fwd_plan_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert " 0 violations" in r.stdout


def test_every_gpu_route_case_is_a_row_of_the_table():
    """tests/test_gpu_pw_fwd_routes.py runs no shape whose route is not pinned."""
    cases = re.findall(r'_case\("([^"]+)"', open(os.path.join(ROOT, "tests", "test_gpu_pw_fwd_routes.py")).read())
    table = open(os.path.join(ROOT, "tests", "pw_fwd_plan_check.cpp")).read()
    rows = set(re.findall(r'^  \{"([^"]+)", "', table, flags=re.M))
    assert len(cases) > 40 and not [c for c in cases if c not in rows]


def test_stat_tiles_is_the_plans_tile_count(lib):
    assert lib.eat_pw_conv_stat_tiles(3, 260, 0) == 4 and lib.eat_pw_conv_stat_tiles(3, 260, 1) == 6
    assert lib.eat_pw_conv_stat_tiles(256, 2000, 0) == 2000 and lib.eat_pw_conv_stat_tiles(70000, 32768, 0) == 8960000


# Requests the entry points refuse with EAT_EINVAL before anything is launched (no GPU needed): one row at least per rule and
# entry point, each the entry point's valid call below with the named arguments changed.  Recorded from the library as it stood
# BEFORE the rules moved into pw_fwd_plan.h: all of them were refused there.
_buf = ctypes.create_string_buffer(64)
P = ctypes.addressof(_buf)
BASE = {
    "eat_pw_conv_fwd": dict(x=P, wp=P, bias=P, in_scale=None, res=None, y=P, pool=None, B=2, Ci=8, Co=24, S=64, act=0, stream=None),
    "eat_pw_conv_bf16_fwd": dict(x=P, wp=P, bias=P, in_scale=None, res=None, y=P, pool=None, B=2, Ci=8, Co=24, S=64, act=0, split=1, stream=None),
    "eat_pw_conv_tf_fwd": dict(x=P, tf_a=P, tf_b=P, tf_act=1, wp=P, wmode=0, bias=P, in_scale=None, res=None, y=P, B=2, Ci=16, Co=24, S=64, act=0, stream=None),
    "eat_pw_conv_cat_fwd": dict(x1=P, C1=8, x2=P, C2=12, wp=P, wmode=0, bias=P, res=None, y=P, B=2, Co=24, S=64, act=0, stream=None),
    "eat_pw_conv_dyn_fwd": dict(x=P, wp_b=P, bias=P, res=None, y=P, B=2, Ci=8, Co=24, S=64, act=0, stream=None),
    "eat_pw_conv_dyn_bf16_fwd": dict(x=P, wp_b=P, bias=P, res=None, y=P, B=2, Ci=8, Co=24, S=64, act=0, stream=None),
    "eat_pw_conv_kcat_fwd": dict(x=P, wp=P, bias=P, att_scale=P, res=None, y=P, B=2, Ci=32, nbank=4, Co=24, S=64, act=0, stream=None),
    "eat_pw_conv_stats_fwd": dict(x=P, wp=P, wmode=0, per_sample=0, tf_a=None, tf_b=None, tf_act=0, in_scale=None, zero_bias=P, y=P, part=P, B=2, Ci=8, Co=24, S=64, stream=None),
    "eat_pw_conv_gstats_fwd": dict(x=P, wp=P, wmode=0, zero_bias=P, y=P, gz=P, g_a=P, g_b=P, g_act=1, part=P, B=2, Ci=8, Co=24, S=64, stream=None),
    "eat_pw_conv_b16_fwd": dict(x=P, x_b16=1, x2=None, c1=0, wp=P, bias=P, tf_a=None, tf_b=None, tf_act=0, in_scale=None, res=None, y=P, y_b16=0, stats_part=None, gz=None, g_a=None, g_b=None, g_act=0, B=2, Ci=32, Co=24, S=64, act=0, stream=None),
    "eat_pw_conv_dyn_b16_fwd": dict(x=P, x_b16=1, wp_b=P, bias=P, res=None, y=P, y_b16=0, stats_part=None, B=2, Ci=8, Co=24, S=64, act=0, stream=None),
}
ROWS = [
    ("eat_pw_conv_fwd", dict(Ci=6)), ("eat_pw_conv_fwd", dict(act=3)), ("eat_pw_conv_fwd", dict(act=-1)), ("eat_pw_conv_fwd", dict(B=0)),
    ("eat_pw_conv_fwd", dict(Ci=0)), ("eat_pw_conv_fwd", dict(Co=0)), ("eat_pw_conv_fwd", dict(S=0)),
    ("eat_pw_conv_bf16_fwd", dict(Ci=6)), ("eat_pw_conv_bf16_fwd", dict(act=3)), ("eat_pw_conv_bf16_fwd", dict(B=0)), ("eat_pw_conv_bf16_fwd", dict(Co=0)),
    ("eat_pw_conv_bf16_fwd", dict(S=0)), ("eat_pw_conv_bf16_fwd", dict(B=70000, S=32768)), ("eat_pw_conv_bf16_fwd", dict(B=70000, S=32768, split=0)),
    ("eat_pw_conv_tf_fwd", dict(tf_a=None)), ("eat_pw_conv_tf_fwd", dict(tf_b=None)), ("eat_pw_conv_tf_fwd", dict(tf_act=3)), ("eat_pw_conv_tf_fwd", dict(act=3)),
    ("eat_pw_conv_tf_fwd", dict(Ci=12)), ("eat_pw_conv_tf_fwd", dict(S=15)), ("eat_pw_conv_tf_fwd", dict(B=0)), ("eat_pw_conv_tf_fwd", dict(Co=0)),
    ("eat_pw_conv_tf_fwd", dict(Ci=12, wmode=2)), ("eat_pw_conv_tf_fwd", dict(S=15, wmode=1)), ("eat_pw_conv_tf_fwd", dict(B=70000, S=32768, wmode=2)),
    ("eat_pw_conv_cat_fwd", dict(x1=None)), ("eat_pw_conv_cat_fwd", dict(x2=None)), ("eat_pw_conv_cat_fwd", dict(C1=0)), ("eat_pw_conv_cat_fwd", dict(C2=2)),
    ("eat_pw_conv_cat_fwd", dict(C1=6)), ("eat_pw_conv_cat_fwd", dict(C2=10)), ("eat_pw_conv_cat_fwd", dict(S=15)), ("eat_pw_conv_cat_fwd", dict(act=3)),
    ("eat_pw_conv_cat_fwd", dict(B=0)), ("eat_pw_conv_cat_fwd", dict(Co=0)), ("eat_pw_conv_cat_fwd", dict(S=15, wmode=2)),
    ("eat_pw_conv_dyn_fwd", dict(Ci=6)), ("eat_pw_conv_dyn_fwd", dict(act=3)), ("eat_pw_conv_dyn_fwd", dict(B=0)), ("eat_pw_conv_dyn_fwd", dict(Ci=0)),
    ("eat_pw_conv_dyn_bf16_fwd", dict(Ci=6)), ("eat_pw_conv_dyn_bf16_fwd", dict(S=15)), ("eat_pw_conv_dyn_bf16_fwd", dict(act=3)), ("eat_pw_conv_dyn_bf16_fwd", dict(B=0)),
    ("eat_pw_conv_dyn_bf16_fwd", dict(Co=0)), ("eat_pw_conv_dyn_bf16_fwd", dict(wp_b=None)),
    ("eat_pw_conv_kcat_fwd", dict(Ci=16)), ("eat_pw_conv_kcat_fwd", dict(Ci=48)), ("eat_pw_conv_kcat_fwd", dict(S=15)), ("eat_pw_conv_kcat_fwd", dict(nbank=0)),
    ("eat_pw_conv_kcat_fwd", dict(B=0)), ("eat_pw_conv_kcat_fwd", dict(Co=0)), ("eat_pw_conv_kcat_fwd", dict(att_scale=None)), ("eat_pw_conv_kcat_fwd", dict(act=3)),
    ("eat_pw_conv_stats_fwd", dict(x=None)), ("eat_pw_conv_stats_fwd", dict(wp=None)), ("eat_pw_conv_stats_fwd", dict(y=None)), ("eat_pw_conv_stats_fwd", dict(part=None)),
    ("eat_pw_conv_stats_fwd", dict(zero_bias=None)), ("eat_pw_conv_stats_fwd", dict(tf_a=P)), ("eat_pw_conv_stats_fwd", dict(tf_b=P)), ("eat_pw_conv_stats_fwd", dict(tf_act=3)),
    ("eat_pw_conv_stats_fwd", dict(tf_a=P, tf_b=P, Ci=12)), ("eat_pw_conv_stats_fwd", dict(Ci=6)), ("eat_pw_conv_stats_fwd", dict(B=0)), ("eat_pw_conv_stats_fwd", dict(B=70000, S=32768, wmode=2)),
    ("eat_pw_conv_gstats_fwd", dict(x=None)), ("eat_pw_conv_gstats_fwd", dict(gz=None)), ("eat_pw_conv_gstats_fwd", dict(g_a=None)), ("eat_pw_conv_gstats_fwd", dict(g_b=None)),
    ("eat_pw_conv_gstats_fwd", dict(part=None)), ("eat_pw_conv_gstats_fwd", dict(zero_bias=None)), ("eat_pw_conv_gstats_fwd", dict(g_act=3)), ("eat_pw_conv_gstats_fwd", dict(wmode=1)),
    ("eat_pw_conv_gstats_fwd", dict(Ci=6)), ("eat_pw_conv_gstats_fwd", dict(B=0)),
    ("eat_pw_conv_b16_fwd", dict(x=None)), ("eat_pw_conv_b16_fwd", dict(wp=None)), ("eat_pw_conv_b16_fwd", dict(bias=None)), ("eat_pw_conv_b16_fwd", dict(y=None)),
    ("eat_pw_conv_b16_fwd", dict(B=0)), ("eat_pw_conv_b16_fwd", dict(Co=0)), ("eat_pw_conv_b16_fwd", dict(Ci=0)), ("eat_pw_conv_b16_fwd", dict(Ci=30)),
    ("eat_pw_conv_b16_fwd", dict(S=4)), ("eat_pw_conv_b16_fwd", dict(S=60)), ("eat_pw_conv_b16_fwd", dict(act=3)), ("eat_pw_conv_b16_fwd", dict(tf_act=3)),
    ("eat_pw_conv_b16_fwd", dict(tf_a=P)), ("eat_pw_conv_b16_fwd", dict(tf_a=P, tf_b=P, Ci=36)), ("eat_pw_conv_b16_fwd", dict(x_b16=0, y_b16=0)),
    ("eat_pw_conv_b16_fwd", dict(x_b16=0, y_b16=1, res=P)), ("eat_pw_conv_b16_fwd", dict(x_b16=0, y_b16=1, in_scale=P)), ("eat_pw_conv_b16_fwd", dict(x_b16=0, y_b16=1, stats_part=P)),
    ("eat_pw_conv_b16_fwd", dict(x_b16=0, y_b16=1, x2=P, c1=32, Ci=40)), ("eat_pw_conv_b16_fwd", dict(x_b16=0, y_b16=1, tf_a=P, tf_b=P)),
    ("eat_pw_conv_b16_fwd", dict(x2=P, c1=16, Ci=40)), ("eat_pw_conv_b16_fwd", dict(x2=P, c1=48, Ci=56)), ("eat_pw_conv_b16_fwd", dict(x2=P, c1=32, Ci=32)),
    ("eat_pw_conv_b16_fwd", dict(x2=P, c1=32, Ci=40, in_scale=P)), ("eat_pw_conv_b16_fwd", dict(x2=P, c1=32, Ci=40, stats_part=P)), ("eat_pw_conv_b16_fwd", dict(x2=P, c1=32, Ci=40, tf_a=P, tf_b=P)),
    ("eat_pw_conv_b16_fwd", dict(y_b16=1, x2=P, c1=32, Ci=40)), ("eat_pw_conv_b16_fwd", dict(y_b16=1, res=P)),
    ("eat_pw_conv_b16_fwd", dict(y_b16=1, gz=P, g_a=P, g_b=P)), ("eat_pw_conv_b16_fwd", dict(y_b16=1, gz=P, g_a=None, g_b=P, stats_part=P)),
    ("eat_pw_conv_b16_fwd", dict(y_b16=1, gz=P, g_a=P, g_b=P, stats_part=P, g_act=3)), ("eat_pw_conv_b16_fwd", dict(y_b16=1, gz=P, g_a=P, g_b=P, stats_part=P, in_scale=P)),
    ("eat_pw_conv_b16_fwd", dict(B=70000, S=32768)),
    ("eat_pw_conv_dyn_b16_fwd", dict(x=None)), ("eat_pw_conv_dyn_b16_fwd", dict(wp_b=None)), ("eat_pw_conv_dyn_b16_fwd", dict(bias=None)), ("eat_pw_conv_dyn_b16_fwd", dict(y=None)),
    ("eat_pw_conv_dyn_b16_fwd", dict(B=0)), ("eat_pw_conv_dyn_b16_fwd", dict(Co=0)), ("eat_pw_conv_dyn_b16_fwd", dict(Ci=6)), ("eat_pw_conv_dyn_b16_fwd", dict(Ci=0)),
    ("eat_pw_conv_dyn_b16_fwd", dict(S=12)), ("eat_pw_conv_dyn_b16_fwd", dict(S=0)), ("eat_pw_conv_dyn_b16_fwd", dict(act=3)), ("eat_pw_conv_dyn_b16_fwd", dict(x_b16=0, y_b16=0)),
    ("eat_pw_conv_dyn_b16_fwd", dict(x_b16=1, y_b16=1)), ("eat_pw_conv_dyn_b16_fwd", dict(x_b16=0, y_b16=1, res=P)),
]


@pytest.mark.parametrize("name,change", ROWS, ids=[f"{n[12:-4]}-{'-'.join(f'{k}={0 if v is None else 1 if v == P else v}' for k, v in c.items())}" for n, c in ROWS])
def test_entry_point_refuses(lib, name, change):
    args = dict(BASE[name])
    assert all(k in args for k in change)
    args.update(change)
    assert getattr(lib, name)(*args.values()) == -1                      # EAT_EINVAL
    assert lib.eat_last_error_string().decode().startswith(name + ":")


@pytest.mark.parametrize("name", ["eat_pw_conv_stats_fwd", "eat_pw_conv_gstats_fwd"])
def test_statistics_entry_points_answer_1_off_the_16_byte_grid(lib, name):
    """S % 4 != 0: the two statistics entry points launch nothing and answer 1 (the caller runs the separate pass)."""
    args = dict(BASE[name], S=15)
    assert getattr(lib, name)(*args.values()) == 1
