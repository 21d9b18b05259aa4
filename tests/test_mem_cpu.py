"""The memory ledger (ekf_vio_amd/csrc/mem.h) without a GPU: tests/mem_ledger_main.cpp, a plain program over a malloc backend, compiled
with the host sanitizers and run; and the two rules the ledger's place in the library rests on, read from the sources."""
import glob
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "ekf_vio_amd", "csrc")
BACKEND_FILE = "api.hip"  # defines hip_mem_backend


def test_ledger_program_runs_clean_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "mem_ledger_main")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                           "-o", exe, os.path.join(HERE, "mem_ledger_main.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    assert r.returncode == 0, r.stdout
    assert "mem ledger: ok" in r.stdout


def test_only_the_backend_calls_the_runtimes_allocation_functions():
    names = re.compile(r"hipMalloc|hipFree|hipHostMalloc|hipHostFree")
    files = sorted(glob.glob(os.path.join(CSRC, "*")))
    assert os.path.join(CSRC, BACKEND_FILE) in files and len(files) > 10
    offenders = [os.path.basename(p) for p in files if os.path.basename(p) != BACKEND_FILE and names.search(open(p).read())]
    assert not offenders, offenders
    # ... and the backend file calls them inside the backend's two functions only
    text = open(os.path.join(CSRC, BACKEND_FILE)).read()
    body = text[text.index("int hip_mem_allocate("):text.index("const MemBackend& hip_mem_backend()")]
    assert len(names.findall(text)) == len(names.findall(body)) > 0


def test_mem_h_includes_standard_headers_only():
    text = open(os.path.join(CSRC, "mem.h")).read()
    includes = re.findall(r"^\s*#\s*include\s*([<\"][^>\"]+[>\"])", text, re.M)
    assert includes
    for inc in includes:
        assert inc.startswith("<") and not inc.startswith("<hip/"), inc  # no project header ("..."), no HIP
    assert "hip_runtime" not in text
