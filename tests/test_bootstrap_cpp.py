"""The C++ layer of the EM bootstrap: a ten-line program calls sbgpu::EmBatch::bootstrap (include/sbgpu_host.hpp).  Without a GPU
it only has to compile and link (as tests/test_abi.py links the C header with gcc); with one it runs, and its numbers are those
of EmBatchSolver.run_bootstrap on the same batch."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LOCI = [([10, 20, 30], [[.1, .2], [.3, .1], [.2, .2]]), ([5, 0, 7, 9], [[.2, 0., .1], [0., .3, .1], [.1, .1, 0.], [.05, .2, .3]])]

PROGRAM = """#include <hip/hip_runtime_api.h>
#include "sbgpu_host.hpp"
int main() {
   sbgpu::Context ctx(0);
   sbgpu::EmBatch b;
%s
   const sbgpu::EmBatch::Bootstrap r = b.bootstrap(ctx, 4, 0x5742, 1, {11, 1ll << 33});
   for (size_t j = 0; j < r.mean.size(); ++j) std::printf("%%a %%a\\n", r.mean[j], r.var[j]);
   for (int32_t c : r.status_count) std::printf("%%d\\n", c);
   return 0;
}
"""


def braces(x):
    return "{" + ", ".join(braces(v) if isinstance(v, list) else repr(v) for v in x) + "}"


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    from strawberry_amd import _lib
    _lib.load()
    d = tmp_path_factory.mktemp("boot_cpp")
    src, exe = d / "boot.cpp", d / "boot"
    src.write_text(PROGRAM % "\n".join("   b.add(%d, %s, %s);" % (len(F[0]), braces(n), braces(F)) for n, F in LOCI))
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I",
                           os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", libdir, "-lsbgpu", "-L", "/opt/rocm/lib",
                           "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_program_builds(program):
    assert os.path.exists(program)


@pytest.mark.gpu
def test_program_gives_the_python_layer_numbers(program):
    from strawberry_amd import em, synth
    out = subprocess.run([str(program)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout, out.stderr)
    lines = out.stdout.split("\n")
    s = em.EmBatchSolver(synth.from_loci([(np.array(n, np.int32), np.array(F)) for n, F in LOCI]))
    r = s.run_bootstrap(4, 0x5742, rep_first=1, locus_id=[11, 1 << 33])
    s.synchronize()
    mean, var = r["mean"].cpu().numpy(), r["var"].cpu().numpy()
    got = np.array([[float.fromhex(x) for x in l.split()] for l in lines[:len(mean)]])
    assert got[:, 0].tobytes() == mean.tobytes() and got[:, 1].tobytes() == var.tobytes()
    assert [int(x) for x in lines[len(mean):] if x] == r["status_count"].cpu().numpy().reshape(-1).tolist()
    assert (var > 0).any()
