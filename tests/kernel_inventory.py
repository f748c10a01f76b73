"""The project's kernels in the built libspt.so, by mangled name (symbol names
only: nothing here reads a kernel's instructions).

Every translation unit's device code sits in the library's .hip_fatbin section
as one clang offload bundle.  The section is cut at the bundles' magic,
clang-offload-bundler takes the gfx950 code object out of each, and
llvm-readelf lists its symbols; a kernel is a symbol NAME with a
kernel-descriptor twin NAME.kd.  Kept: the kernels of namespace spt (mangled
_ZN3spt...) and the ones named in EXTRA.  Left out: rocprim / hipcub kernels
(namespace rocprim) and the runtime's __amd_rocclr_* helpers.

    python tests/kernel_inventory.py            # one mangled name per line
"""
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "smallpt-enoki-optix_amd", "build", "libspt.so")
BUILD_HINT = 'python -c "import __graft_entry__ as g; g.build()"   (from the repository root)'
ARCH = "gfx950"
TARGET = "hipv4-amdgcn-amd-amdhsa--" + ARCH
BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
# project kernels outside namespace spt (mangled names): none today
EXTRA = ()


class InventoryError(RuntimeError):
    pass


def _tool(name):
    for d in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin"),
              os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin")):
        p = os.path.join(d, name)
        if os.access(p, os.X_OK):
            return p
    p = shutil.which(name)
    if not p:
        raise InventoryError(f"{name} not found (ROCm's llvm/bin)")
    return p


def _run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise InventoryError(f"{' '.join(cmd)} failed ({r.returncode}): {r.stderr.strip()[-400:]}")
    return r.stdout


def _fatbin_section(lib):
    """(file offset, size) of .hip_fatbin, from llvm-readelf's section table."""
    for line in _run([_tool("llvm-readelf"), "--sections", "--wide", lib]).splitlines():
        f = line.replace("[", " ").replace("]", " ").split()
        if len(f) >= 6 and f[1] == ".hip_fatbin":
            return int(f[4], 16), int(f[5], 16)
    raise InventoryError(f"{lib} has no .hip_fatbin section")


def code_objects(lib=LIB, outdir=None):
    """Paths of the gfx950 code objects of `lib`, one per bundle, in section order."""
    if not os.path.exists(lib):
        raise InventoryError(f"{lib} is not built; build it with: {BUILD_HINT}")
    off, size = _fatbin_section(lib)
    with open(lib, "rb") as f:
        f.seek(off)
        blob = f.read(size)
    starts = []
    at = blob.find(BUNDLE_MAGIC)
    while at >= 0:
        starts.append(at)
        at = blob.find(BUNDLE_MAGIC, at + len(BUNDLE_MAGIC))
    if not starts:
        raise InventoryError(f"{lib}: no offload bundle in .hip_fatbin (compressed bundles are not supported)")
    out = []
    bundler = _tool("clang-offload-bundler")
    for k, (a, b) in enumerate(zip(starts, starts[1:] + [len(blob)])):
        piece = os.path.join(outdir, f"bundle{k}.hipfb")
        with open(piece, "wb") as f:
            f.write(blob[a:b])
        targets = _run([bundler, "--list", "--type=o", f"--input={piece}"]).split()
        if TARGET not in targets:
            continue  # a translation unit without device code for this arch
        co = os.path.join(outdir, f"bundle{k}.{ARCH}.co")
        _run([bundler, "--unbundle", "--type=o", f"--targets={TARGET}", f"--input={piece}", f"--output={co}"])
        out.append(co)
    if not out:
        raise InventoryError(f"{lib}: no {ARCH} code object")
    return out


def kernel_symbols(code_object):
    """Every NAME that has a NAME.kd kernel descriptor in the code object."""
    names = set()
    for line in _run([_tool("llvm-readelf"), "--symbols", "--wide", code_object]).splitlines():
        f = line.split()
        if len(f) >= 8 and f[-1].endswith(".kd"):
            names.add(f[-1][:-3])
    return names


def is_project_kernel(name):
    return name.startswith("_ZN3spt") or name in EXTRA


def all_kernels(lib=LIB):
    """Every kernel of the library, the runtime's and rocprim's included."""
    with tempfile.TemporaryDirectory() as tmp:
        names = set()
        for co in code_objects(lib, tmp):
            names |= kernel_symbols(co)
    return names


def project_kernels(lib=LIB):
    """The sorted mangled names of the project's kernels in the built library."""
    return sorted(n for n in all_kernels(lib) if is_project_kernel(n))


if __name__ == "__main__":
    try:
        ks = project_kernels()
    except InventoryError as e:
        sys.exit(str(e))
    print("\n".join(ks))
    print(f"{len(ks)} project kernels", file=sys.stderr)
