"""The slot refusals and event-row walks that the ragged-bank kernels share (efficientat_amd/csrc/event_bank.h) without a GPU:
a stand-alone checker (tests/event_bank_check.cpp) built with AddressSanitizer and UBSan compares them with brute force on
small banks whose tables are exact-size heap arrays, so "nothing outside the bank is read" is checked on memory itself."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_event_bank_helpers_under_sanitizers(tmp_path):
    # the sanitizer runtimes are linked statically: the program then runs the same whatever the environment preloads
    gxx = shutil.which("g++")
    cmd = [gxx, "-static-libasan", "-static-libubsan"] if gxx else [shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++", "-static-libsan"]
    exe = str(tmp_path / "event_bank_check")
    subprocess.run(cmd + ["-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                          "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "efficientat_amd", "csrc"),
                          os.path.join(ROOT, "tests", "event_bank_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert " 0 violations" in r.stdout
