"""The IK scratch-set scheduler (kinematics.jl_amd/csrc/kinhip_ik_sets.h) on the host alone (CPU only).

`make -C kinematics.jl_amd/csrc ik-sets-check` builds tests/host/ik_sets_check.cpp -- the scheduler over a fake
runtime backend, with the host compiler, no HIP and no device code -- once under ThreadSanitizer and once under
ASan + UBSan.  The program runs the deterministic cases of the policy (which set a call gets, when it waits on the
host, what it counts, captures, the event-error paths, a dropped lease, a failed record) at the real set counts,
then 8 threads against a "device" thread; a failed check or any sanitizer report fails it."""
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "kinematics.jl_amd", "csrc")
HOST = os.path.join(ROOT, "kinematics.jl_amd", "lib", "host")


@pytest.fixture(scope="module")
def built():
    subprocess.check_call(["make", "-s", "-C", CSRC, "ik-sets-check"])
    return HOST


@pytest.mark.parametrize("variant", ["tsan", "asan"])
def test_ik_sets_check(built, variant):
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1", ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1")
    # the hard time limit is the lost-wake-up check: the threaded case must end
    r = subprocess.run([os.path.join(built, "ik_sets_check_" + variant)], env=env, capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "ik_sets_check: ok" in r.stdout
