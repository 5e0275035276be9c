"""The resource owners of the host layer (csrc/lh_hip_own.h) on the CPU: tests/host_own/own_check.cpp, a stand-alone
program, exercises them against a stand-in <hip/hip_runtime.h> that keeps a table of what is live and aborts on a release
of anything that is not."""
import os
import subprocess

import helpers


def test_hip_owners_release_exactly_what_they_hold(tmp_path):
    here = os.path.join(helpers.ROOT, "tests", "host_own")
    exe = str(tmp_path / "own_check")
    # (the stand-in header's directory first: it is the only <hip/hip_runtime.h> this build may see)
    subprocess.check_call(["g++", "-std=c++17", "-I" + here, "-I" + os.path.join(helpers.ROOT, "deprecated-lame-mirror_amd", "csrc"),
                           os.path.join(here, "own_check.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
