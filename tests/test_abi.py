"""The C-ABI shared library loads on a CPU-only box and exports every symbol that
include/flye_gpu.h declares.  No compute call is made here."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header="flye_gpu.h", prefix="fg_"):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(" + prefix + r"[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_exported(built):
    from flye_amd import gpu
    lib = gpu.load_library()
    names = _declared()
    assert len(names) >= 12
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/flye_gpu.h but not exported"
    assert set(gpu.ABI_SYMBOLS) <= set(names)
    assert lib.fg_abi_version() == 4
    # the batch scheduler above the ABI (include/flye_gpu_bridge.h)
    bridge = _declared("flye_gpu_bridge.h", "fgb_")
    assert len(bridge) >= 8
    for n in bridge:
        assert hasattr(lib, n), f"{n} declared in include/flye_gpu_bridge.h but not exported"
    assert lib.fgb_create(None, None, None, 0, 0) == -3


def test_error_strings_and_argument_checks(built):
    from flye_amd import gpu
    lib = gpu.load_library()
    assert lib.fg_strerror(0) == b"ok"
    assert b"CPU" in lib.fg_strerror(-1)
    h = C.c_void_p()
    assert lib.fg_create(C.byref(h), 0, 33) == -6      # k > 32 never fits KmerRepr
    assert lib.fg_create(None, 0, 17) == -3


def test_no_cpu_fallback_without_device(built):
    """Without a HIP device the product must fail loudly, not fall back."""
    import torch
    from flye_amd import gpu
    if torch.cuda.is_available():
        return
    try:
        gpu.Context(17, 0)
    except gpu.FlyeGpuError as e:
        assert e.code == -1
    else:
        raise AssertionError("Context() succeeded without a GPU")


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "flye_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".cpp", ".h")) or f == "Makefile":
                src = open(os.path.join(dirpath, f)).read()
                for pat in (r"import\s+oracle", r"from\s+oracle", r"liboracle", r"oracle/", r"fo_[a-z_]+\("):
                    assert not re.search(pat, src), f"{f} reaches into the test oracle ({pat})"


def _build_c_demo(tmp_path):
    import subprocess
    exe = str(tmp_path / "c_abi_demo")
    lib = os.path.join(ROOT, "flye_amd", "lib")
    subprocess.run(["gcc", "-std=c99", "-pthread", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "c_abi_demo.c"), "-L" + lib, "-lflyegpu",
                    "-Wl,-rpath," + lib, "-o", exe], check=True)
    return exe


def test_header_is_plain_c_and_links(built, tmp_path):
    """include/flye_gpu.h compiles as C99 and a C program links against the library; without
    a GPU the program reports FG_ERR_NO_DEVICE (exit status 2)."""
    import subprocess
    import torch
    exe = _build_c_demo(tmp_path)
    if not torch.cuda.is_available():
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 2 and "no usable HIP device" in r.stdout


import pytest  # noqa: E402


@pytest.mark.gpu
def test_c_consumer_runs_on_gpu(built, tmp_path):
    import subprocess
    exe = _build_c_demo(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "overlaps for 60 reads" in r.stdout and "scheduler:" in r.stdout


def test_graft_entry_build_passes(built):
    """build() is the driver's "does it build" check: it must succeed on a CPU-only box
    (a stale assertion in it once outlived an ABI bump)."""
    import sys
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build()


@pytest.mark.gpu
def test_context_creation_leaves_libc_rand_stream_alone(built):
    """HIP runtime initialisation draws from libc's rand(); fg_create shields the caller's stream, which
    the reference relies on for the reads estimateOverlaperParameters picks (overlap.cpp:752-756).
    Runs in a fresh process so that this really is the first runtime initialisation."""
    import subprocess
    import sys
    code = ("import ctypes, sys; sys.path.insert(0, %r); from flye_amd import gpu; libc = ctypes.CDLL(None); "
            "libc.srand(1); c = gpu.Context(17, 0); print(libc.rand())") % ROOT
    out = subprocess.run([sys.executable, "-c", code], check=True, capture_output=True, text=True)
    assert int(out.stdout.split()[-1]) == 1804289383     # glibc: first value of the stream seeded with 1


def test_every_device_primitive_is_ours(built):
    """north_star asks for hand-written kernels: the library's code objects hold no rocPRIM / hipCUB / Thrust kernel
    (their template instantiations would carry those namespaces in the kernel names embedded in the .so), and the
    sources include none of those headers."""
    so = os.path.join(ROOT, "flye_amd", "lib", "libflyegpu.so")
    blob = open(so, "rb").read().lower()
    for lib_name in (b"rocprim", b"hipcub", b"thrust"):
        assert lib_name not in blob, f"{lib_name.decode()} kernels inside libflyegpu.so"
    src = os.path.join(ROOT, "flye_amd", "csrc")
    for f in os.listdir(src):
        if f.endswith((".hip", ".h", ".cpp")):
            text = open(os.path.join(src, f)).read()
            assert not re.search(r"#include\s*<(rocprim|hipcub|thrust)/", text), f
