"""Device and pinned host memory is owned by type (csrc/devmem.hpp: Dev<T>, DevGrow, Pinned<T>): no other file of csrc/ calls the runtime
functions that allocate or release it, so a buffer cannot outlive its owner by a forgotten line in a destructor.  No GPU needed."""
import os
import re
import shutil
import subprocess


CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "cup3d_amd", "csrc")
# hipMalloc, hipFree, hipHostMalloc, hipHostFree and their relatives (hipMallocAsync, hipHostAlloc, ...), as calls
CALL = re.compile(r"\bhip\w*(?:Malloc|Free|HostAlloc)\w*\s*\(")

# The process-lifetime objects: no heap object with an explicit destroy call holds them, and an owner of static storage duration would
# free them after the HIP runtime has been torn down.  They stay raw pointers, released where they always were.
ALLOWED = {
    ("poisson_block.hpp", "g_invD"): 1,     # the block solve's eigenvalue table: allocated on first use, never freed
    ("comm.hip", "d_flag"): 2,              # g_comm's all-reduce flag: allocated by the first agree(), freed by cup3d_comm_finalize
}


def _code(text):
    """the file without // comments (a comment may speak of hipMalloc)"""
    return "\n".join(line.split("//")[0] for line in text.splitlines())


def test_only_devmem_hpp_allocates_and_releases():
    found = {}
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith((".hip", ".hpp", ".cpp", ".h")) or name == "devmem.hpp":
            continue
        with open(os.path.join(CSRC, name)) as f:
            for n, line in enumerate(_code(f.read()).splitlines(), 1):
                if CALL.search(line):
                    key = next((k for k in ALLOWED if k[0] == name and k[1] in line), None)
                    assert key is not None, f"{name}:{n} allocates or releases outside devmem.hpp: {line.strip()}"
                    found[key] = found.get(key, 0) + 1
    assert found == ALLOWED   # ... and the allow-list names nothing that is gone
    with open(os.path.join(CSRC, "devmem.hpp")) as f:
        own = _code(f.read())
    for fn in ("hipMalloc", "hipFree", "hipHostMalloc", "hipHostFree"):
        assert re.search(r"\b%s\s*\(" % fn, own), fn


def test_no_owner_has_static_storage():
    """a namespace-scope or static Dev / DevGrow / Pinned would be destroyed after the runtime"""
    bad = re.compile(r"^\s*(?:static|thread_local|extern)\b[^;(]*\b(?:Dev<|DevGrow\b|Pinned<)|^(?:Dev<|DevGrow\b|Pinned<)[^;(]*;", re.M)
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".hpp", ".cpp")) and name != "devmem.hpp":
            with open(os.path.join(CSRC, name)) as f:
                m = bad.search(_code(f.read()))
            assert m is None, f"{name}: {m.group(0).strip()}"


def test_the_owners_static_asserts_hold(tmp_path):
    """devmem.hpp stands alone and its static_asserts (move-only, nothrow-movable, converts to T*) are evaluated by a host compile"""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"   # the compiler csrc/Makefile builds the library with
    tu = tmp_path / "owner.cpp"
    tu.write_text('#include "devmem.hpp"\nstatic_assert(sizeof(cup3d::Dev<double>) == 2 * sizeof(void *), "a pointer and a count");\nint main() { return 0; }\n')
    r = subprocess.run([hipcc, "-std=c++17", "-fsyntax-only", "-I", CSRC, "-x", "hip", "--offload-host-only", str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
