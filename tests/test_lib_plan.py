"""The pure pieces of the library path's host code (csrc/shs_lib_plan.hpp: build_rt_order, build_draw_table,
plan_lib_pass, shadow_covers / shadow_union) on the CPU: tests/lib_plan's stand-alone program, compiled with
the address and undefined-behaviour sanitizers, linking neither HIP nor libshs_gpu.so."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PLAN = os.path.join(ROOT, "tests", "lib_plan")
EXE = os.path.join(LIB_PLAN, "_build", "lib_plan_test")


def test_lib_plan_pure_pieces():
    subprocess.run(["make", "-s", "-C", LIB_PLAN], check=True)
    r = subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
