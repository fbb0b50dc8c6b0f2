"""The host front that the batched resident-cloud entry points share (csrc/cloud_batch.hpp, voxel_grid.hpp,
cell_sort.hpp: the range recorder, the compacting front and finish, the parts of the scratch tail, table_slots, the
argument checks) as a stand-alone C++ program, tests/cpp/cloud_batch_host_test.cpp: compiled for the host alone with
AddressSanitizer and UndefinedBehaviorSanitizer and run in a child process.  It links no library and touches no device;
every address in it is made up and never dereferenced."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_front_of_the_batched_cloud_calls_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "cloud_batch_host_test")
    build = subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "-static-libasan", "-static-libubsan",  # the runtimes linked in: the program does not depend on the order in which libraries load
         "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "align3d_amd", "csrc"),
         os.path.join(ROOT, "tests", "cpp", "cloud_batch_host_test.cpp"), "-o", exe],
        capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    tail = (run.stdout + run.stderr)[-4000:]
    assert run.returncode == 0, tail
    assert "cloud_batch_host_test: ok" in run.stdout and "runtime error" not in tail and "AddressSanitizer" not in tail, tail
