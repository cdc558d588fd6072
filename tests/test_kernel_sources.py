"""Two places must know every file the kernels are compiled from: the cache key
of the specialised code objects (mgs.core.special.SOURCES) and the staleness
test of the libraries' per-unit objects (__graft_entry__._library_jobs).  Both
derive their lists from the quoted #includes of the translation units; a file
missing from either would mean stale objects reused after an edit.  The case
that matters -- a header added to the kernel source -- is played through on a
copy of csrc/ and include/.  The stage headers that mgs_kernels.hip includes
(mgs_k_*.h), in dependency order, are guarded and include what they use: each
alone passes the compiler's device-side syntax check (about a second each;
the only compiler run here).
No library, nothing on the GPU.
"""
import os
import re
import shutil
import subprocess

import pytest

import __graft_entry__ as entry
from mgs.core import abi, special

UNITS = ["mgs_special.hip", "mgs_inst.hip", "mgs_capi.hip"]


def quoted_includes(path):
    """(independent of the code under test) the quoted includes of one file"""
    with open(path) as f:
        return re.findall(r'^\s*#\s*include\s+"([^"]+)"', f.read(), re.M)


def reachable(unit, csrc=special.CSRC):
    """paths relative to csrc of everything `unit` includes, by this module's
    own reading of the includes"""
    seen, todo = [], [unit]
    while todo:
        rel = os.path.normpath(todo.pop())
        if rel not in seen:
            seen.append(rel)
            todo += [os.path.join(os.path.dirname(rel), i) for i in quoted_includes(os.path.join(csrc, rel))]
    return sorted(seen)


# what a specialised object is compiled from, relative to csrc/
SPECIAL_FILES = reachable("mgs_special.hip")


def check_unit_closure(unit, csrc):
    """the closure of `unit` in the source directory `csrc`: the unit first,
    no file twice, every kernel header of the directory (mgs_k_*.h) in it, and
    every quoted include of every file resolved to a file of the closure"""
    closure = special.include_closure(unit, csrc)
    assert closure[0] == os.path.join(csrc, unit)
    assert len(set(closure)) == len(closure)
    for f in sorted(os.listdir(csrc)):
        if f.startswith("mgs_k_") and f.endswith(".h"):
            assert os.path.join(csrc, f) in closure, f"{f} is not reached from {unit}"
    for path in closure:
        for inc in quoted_includes(path):
            target = os.path.normpath(os.path.join(os.path.dirname(path), inc))
            assert os.path.isfile(target), f"{path} includes {inc}: not found"
            assert target in closure, f"{path} includes {inc}: not in the closure of {unit}"
    return closure


@pytest.mark.parametrize("unit", UNITS)
def test_unit_closure(unit):
    closure = check_unit_closure(unit, special.CSRC)
    assert sorted(closure) == sorted(os.path.normpath(os.path.join(special.CSRC, f)) for f in reachable(unit))
    assert os.path.join(special.CSRC, "mgs_kernels.hip") in closure
    assert os.path.normpath(abi.HEADER) in closure


def test_special_sources_is_the_closure():
    assert special.SOURCES == special.include_closure("mgs_special.hip")
    assert os.path.normpath(abi.HEADER) in special.SOURCES
    assert sorted(special.SOURCES) == sorted(os.path.normpath(os.path.join(special.CSRC, f)) for f in SPECIAL_FILES)


@pytest.mark.parametrize("unit", UNITS)
def test_build_entry_closure_is_the_same_function(unit):
    assert entry._include_closure(unit) == special.include_closure(unit)


def test_build_entry_dependency_lists():
    for name, nvs, defs in (("libmgs_gpu", entry.NV_MAIN, []), ("libmgs_gpu_wide", entry.NV_WIDE, ["-DMGS_WIDE"])):
        jobs, _, _, _ = entry._library_jobs(name, nvs, defs)
        assert len(jobs) == 1 + len(nvs)
        for out, deps, cmd in jobs:
            unit = "mgs_capi.hip" if os.path.basename(out) == "capi.o" else "mgs_inst.hip"
            assert os.path.join(special.CSRC, unit) in cmd
            assert deps == special.include_closure(unit), out


def copy_sources(root):
    """csrc/ and include/ copied under `root` with their relative position kept"""
    csrc = os.path.join(root, "mj-grasp-sim_amd", "csrc")
    shutil.copytree(special.CSRC, csrc)
    shutil.copytree(os.path.dirname(abi.HEADER), os.path.join(root, "include"))
    return csrc


@pytest.fixture(scope="module")
def source_copy(tmp_path_factory):
    return copy_sources(str(tmp_path_factory.mktemp("src")))


@pytest.fixture()
def no_compiler(monkeypatch):
    monkeypatch.setattr(special, "_COMPILER_ID", "no compiler run")


def key_changes_with(path, sources):
    """whether one byte appended to `path` changes the key; `path` is restored"""
    before = special.toolchain_key(special.FLAGS, sources)
    with open(path, "rb") as f:
        kept = f.read()
    try:
        with open(path, "ab") as f:
            f.write(b"\n")
        changed = special.toolchain_key(special.FLAGS, sources) != before
    finally:
        with open(path, "wb") as f:
            f.write(kept)
    assert special.toolchain_key(special.FLAGS, sources) == before
    return changed


@pytest.mark.parametrize("source", SPECIAL_FILES)
def test_a_byte_in_any_source_changes_the_key(source_copy, source, no_compiler):
    sources = special.include_closure("mgs_special.hip", source_copy)
    assert [os.path.relpath(p, source_copy) for p in sources] == \
        [os.path.relpath(p, special.CSRC) for p in special.SOURCES]
    # the copy hashes like the tree itself
    assert special.toolchain_key(special.FLAGS, sources) == special.toolchain_key(special.FLAGS)
    assert key_changes_with(os.path.normpath(os.path.join(source_copy, source)), sources)


# where a header added to the kernel source may be included from
INCLUDERS = ["mgs_kernels.hip", "mgs_k_math.h", "mgs_k_constraints.h", "mgs_launch.h", "../../include/mgs_gpu.h"]


@pytest.mark.parametrize("includer", INCLUDERS)
def test_a_header_added_to_the_kernel_source_is_picked_up(tmp_path, includer, no_compiler):
    """the real sources with one more header, included from `includer`: every
    unit that reaches the includer gets the header into its closure (the
    build's lists too), and the cache key follows its content"""
    csrc = copy_sources(str(tmp_path))
    inc_path = os.path.normpath(os.path.join(csrc, includer))
    new = os.path.join(os.path.dirname(inc_path), "mgs_k_added.h")
    key_before = special.toolchain_key(special.FLAGS, special.include_closure("mgs_special.hip", csrc))
    with open(new, "w") as f:
        f.write("#pragma once\n")
    with open(inc_path) as f:
        text = f.read()
    with open(inc_path, "w") as f:
        f.write('#include "mgs_k_added.h"\n' + text)
    users = [u for u in UNITS if os.path.relpath(inc_path, csrc) in reachable(u, csrc)]
    assert users, includer
    for unit in UNITS:
        for closure in (special.include_closure, entry._include_closure):
            assert (new in closure(unit, csrc)) == (unit in users), (unit, closure)
    if "mgs_special.hip" in users:
        sources = special.include_closure("mgs_special.hip", csrc)
        assert special.toolchain_key(special.FLAGS, sources) != key_before
        assert key_changes_with(new, sources)


def test_a_kernel_header_nobody_includes_is_reported(tmp_path):
    """an mgs_k_*.h file in csrc/ that no unit reaches fails check_unit_closure"""
    csrc = copy_sources(str(tmp_path))
    check_unit_closure("mgs_inst.hip", csrc)
    with open(os.path.join(csrc, "mgs_k_orphan.h"), "w") as f:
        f.write("#pragma once\n")
    with pytest.raises(AssertionError, match="mgs_k_orphan.h is not reached"):
        check_unit_closure("mgs_inst.hip", csrc)


STAGE_HEADERS = sorted(f for f in os.listdir(special.CSRC) if f.startswith("mgs_k_") and f.endswith(".h"))


def test_every_stage_header_is_included_once_by_the_kernel_source():
    """mgs_kernels.hip includes each mgs_k_*.h of csrc/ itself, exactly once, so
    the order of definitions is the order of its include lines"""
    assert STAGE_HEADERS
    included = quoted_includes(os.path.join(special.CSRC, "mgs_kernels.hip"))
    for h in STAGE_HEADERS:
        assert included.count(h) == 1, h


def test_the_include_order_is_a_dependency_order():
    """a stage header includes only stage headers that stand before it in
    mgs_kernels.hip, so every definition is seen at its place in that list
    whichever header is included first"""
    order = [h for h in quoted_includes(os.path.join(special.CSRC, "mgs_kernels.hip")) if h in STAGE_HEADERS]
    assert sorted(order) == STAGE_HEADERS
    for h in STAGE_HEADERS:
        for inc in quoted_includes(os.path.join(special.CSRC, h)):
            if inc in STAGE_HEADERS:
                assert order.index(inc) < order.index(h), f"{h} includes {inc}, which stands after it"


@pytest.mark.parametrize("header", STAGE_HEADERS)
def test_a_stage_header_is_guarded(header):
    with open(os.path.join(special.CSRC, header)) as f:
        assert re.search(r"^#\s*pragma\s+once\s*$", f.read(), re.M), header


def _hipcc():
    for c in ("/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.isfile(c):
            return c
    return None


@pytest.mark.parametrize("flavour", [[], ["-DMGS_WIDE"]], ids=["main", "wide"])
@pytest.mark.parametrize("header", STAGE_HEADERS)
def test_a_stage_header_compiles_alone(source_copy, tmp_path, header, flavour):
    """a unit of one line, the header's include, passes the device-side syntax
    check: the header includes what it uses"""
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("no hipcc")
    unit = os.path.join(source_copy, f"alone_{os.path.basename(str(tmp_path))}.hip")
    with open(unit, "w") as f:
        f.write(f'#include "{header}"\n')
    try:
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++17", "--cuda-device-only", "-fsyntax-only",
                            *flavour, "-I", os.path.join(os.path.dirname(os.path.dirname(source_copy)), "include"),
                            unit], capture_output=True, text=True)
    finally:
        os.remove(unit)
    assert r.returncode == 0, r.stderr[-3000:]


@pytest.mark.parametrize("closure", [special.include_closure, entry._include_closure])
def test_closure_follows_nested_and_relative_includes(tmp_path, closure):
    """a header reached only through another one, in another directory, and
    included twice; angle-bracket and macro includes are not followed"""
    files = {"a.hip": '#include <hip/hip_runtime.h>\n#include "one.h"\n  # include "sub/two.h"\n#include MGS_SPECIAL\n',
             "one.h": '#pragma once\n#include "sub/two.h"\n',
             "sub/two.h": '#include "../three.h"\n// #include "never.h"\n',
             "three.h": "int x;\n"}
    for rel, text in files.items():
        p = tmp_path / rel
        p.parent.mkdir(exist_ok=True)
        p.write_text(text)
    got = closure("a.hip", str(tmp_path))
    assert got == [str(tmp_path / f) for f in ("a.hip", "one.h", "sub/two.h", "three.h")]
    (tmp_path / "three.h").unlink()
    with pytest.raises(OSError):
        closure("a.hip", str(tmp_path))
