"""The staging plan of the diagnostics' host-array entries (kid_amd/csrc/kidmp_stage_plan.h) without a GPU: the header has
nothing of HIP in it, so tests/native/stage_plan_check.cpp enumerates its arithmetic as a host program under ASan + UBSan --
slots aligned, disjoint and inside the planned total, chunks tiling the batch, every copy inside its array and its slot;
chunk and staging bytes of one representative call per entry equal to the entry's former formula; the largest chunk that
fits below an entry's cap -- and every host entry of the units goes through that plan, none past it."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kid_amd", "csrc")
# the units whose *_host bodies stand on the plan, and the bodies
HOST_BODIES = {"kidmp_host.hip": ("refl_host", "radii_host"), "kidmp_summary.hip": ("summary_host",), "kidmp_fall.hip": ("fall_host",),
               "kidmp_doppler.hip": ("doppler_host",), "kidmp_spectra.hip": ("spectra_host",), "kidmp_dspectrum.hip": ("dspectrum_host",),
               "kidmp_lidar.hip": ("lidar_host",), "kidmp_brightband.hip": ("brightband_host",), "kidmp_mie.hip": ("mie_host",),
               "kidmp_radiometer.hip": ("rad_host",), "kidmp_polarimetric.hip": ("pol_host",),
               "kidmp_multichannel.hip": ("rad_multi_host", "mie_multi_host")}


def test_plan_arithmetic_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler"
    exe = tmp_path / "stage_plan_check"
    # the sanitizers' runtimes are linked statically: the program is instrumented by itself and runs in the environment as it is
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx) == "g++" else ["-static-libsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
                   + static + ["-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "native", "stage_plan_check.cpp"),
                               "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip().endswith("stage plan ok") and "runtime error" not in run.stderr, run.stdout + run.stderr


def test_the_makefile_target_runs_it_too():
    r = subprocess.run(["make", "-C", CSRC, "asan-stage-plan"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "stage plan ok" in r.stdout and "runtime error" not in r.stderr, r.stdout[-3000:] + r.stderr[-3000:]


def test_the_plan_header_has_nothing_of_hip():
    text = open(os.path.join(CSRC, "kidmp_stage_plan.h")).read()
    assert re.findall(r"#include\s*[<\"]([^>\"]+)", text) == ["cstddef", "cstdint"]
    code = re.sub(r"//[^\n]*", " ", text)
    assert not re.search(r"\bhip[A-Z_]\w*|__device__|__host__|__global__", code)


def _body(text, name):
    """The text of `int name(...) { ... }`, the template's definition in its unit."""
    m = re.search(r"^int " + name + r"\(", text, flags=re.M)
    assert m, name
    start = text.index("\n{\n", m.start())
    return text[start:text.index("\n}\n", start)]


def test_no_host_body_stages_by_hand():
    for unit, names in HOST_BODIES.items():
        text = open(os.path.join(CSRC, unit)).read()
        for name in names:
            body = _body(text, name)
            assert "stage_plan(" in body and "stage_open(" in body and "stage_run(" in body, (unit, name)
            for word in ("hipMemcpyAsync", "hipMemcpy2DAsync", "hipStreamSynchronize", "ensure_stage", "->d_stage", "/ 256 * 256", "up256"):
                assert word not in body, (unit, name, word)
