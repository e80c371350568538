"""CPU: the C-ABI library loads without a GPU and exports every function include/*.h declares.

No compute call is made here (there is no GPU in the build container); the GPU tests drive the
same entry points."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "gemma.ggml_amd", "lib", "libgemma_hip.so")


def _declared_functions():
    names = []
    for hdr in ("gemma_hpc.h", "ggml.h"):
        text = open(os.path.join(ROOT, "include", hdr)).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        text = re.sub(r"//[^\n]*", "", text)
        for m in re.finditer(r"^\s*[A-Za-z_][\w\s\*]*?\b([A-Za-z_]\w*)\s*\(", text, flags=re.M):
            name = m.group(1)
            line = text[m.start():text.find("\n", m.start())]
            if line.lstrip().startswith(("typedef", "#", "return")) or "(*" in line:
                continue
            if name in ("void", "int", "float", "double", "char", "sizeof", "if", "while", "for"):
                continue
            names.append(name)
    return sorted(set(names))


@pytest.fixture(scope="module")
def lib_path():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-s", "-j8", "-C", os.path.join(ROOT, "gemma.ggml_amd")], check=True)
    return LIB


def test_header_parse_finds_the_boundary():
    names = _declared_functions()
    for must in ("mul_mat", "hpc_init", "hpc_last_error", "gemma_engine_create", "gemma_engine_step",
                 "gemma_test_rope_kv_prefill", "gemma_test_rows_rope_kv", "gemma_test_attn_prefill"):
        assert must in names, names


def test_library_loads_and_exports_all_declared_symbols(lib_path):
    C.CDLL(lib_path)  # loads without a GPU (libamdhip64 resolves; nothing is called)
    out = subprocess.run(["nm", "-D", "--defined-only", lib_path], check=True, capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    missing = [n for n in _declared_functions() if n not in exported]
    assert not missing, f"declared in include/*.h but not exported: {missing}"


def test_python_binding_export_list_is_declared():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "gemma.ggml_amd", "python"))
    import gemma_hip
    declared = set(_declared_functions())
    assert set(gemma_hip.EXPORTS) <= declared, set(gemma_hip.EXPORTS) - declared


def test_product_has_no_cpu_fallback_to_the_oracle(lib_path):
    """The product library must not link or embed the oracle (test infrastructure only)."""
    out = subprocess.run(["nm", "-D", lib_path], check=True, capture_output=True, text=True).stdout
    assert "orc_" not in out
    deps = subprocess.run(["ldd", lib_path], capture_output=True, text=True).stdout
    assert "liboracle" not in deps
