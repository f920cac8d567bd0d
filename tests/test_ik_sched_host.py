"""The IK launch schedule (kinematics.jl_amd/csrc/kinhip_ik_sched.h) on the host alone (CPU only).

`make -C kinematics.jl_amd/csrc ik-sched-check` builds tests/host/ik_sched_check.cpp -- the policy that lays a
kin_ik_dls_batch chunk (and a collision-aware IK call) out on the chip, with the host compiler, no HIP and no device
code -- under ASan + UBSan.  The program asserts the decision field by field for hand-derived cases (bench config 4,
the 1M-target leg, every threshold from both sides, every knob away from its default) and counts the occupancy
questions the policy asks; a failed check or any sanitizer report fails it.  The GPU tests of this path check that
every schedule gives the same answers; this one pins which schedule a call gets."""
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "kinematics.jl_amd", "csrc")
HOST = os.path.join(ROOT, "kinematics.jl_amd", "lib", "host")


def test_ik_sched_check():
    subprocess.check_call(["make", "-s", "-C", CSRC, "ik-sched-check"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(HOST, "ik_sched_check_asan")], env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "ik_sched_check: ok" in r.stdout
