"""pq::Stream and pq::Event (piqp_amd/csrc/common.hpp) own every hipStream_t and hipEvent_t of the library.  Their logic -- construct / move / release / destroy, a
constructor that throws after the handle exists, the order in which a handle type's members go -- is host code: tests/c/stream_raii_kat.cpp instantiates them with
create / destroy pairs that only count, and is built with the address and undefined-behaviour sanitizers.  No GPU needed."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM_INC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


def test_stream_holder_known_answers(tmp_path):
    exe = tmp_path / "stream_raii_kat"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
                    f"-I{ROCM_INC}", os.path.join(ROOT, "tests", "c", "stream_raii_kat.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "all checks passed" in r.stdout
