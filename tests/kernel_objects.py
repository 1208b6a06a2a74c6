"""What the built library's gfx950 kernels look like, read without a GPU: the code objects inside libsdfgrid.so unbundled with
the LLVM binary tools, their metadata notes as a table, and the disassembly of one kernel.  Shared by tests/test_abi.py,
tests/test_program_cpu.py and tools/kernel_diff.py."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM_TOOLS = "/opt/rocm/lib/llvm/bin"


def have_llvm_tools():
    return all(os.path.exists(os.path.join(LLVM_TOOLS, t)) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf", "llvm-objdump"))


def bare_code_object(co):
    """One gfx950 code object that is a file of its own (sdfv_program_compiled_code), in unbundle()'s form."""
    notes = subprocess.run([f"{LLVM_TOOLS}/llvm-readelf", "--notes", str(co)], check=True, capture_output=True, text=True).stdout
    return [(co, notes)]


def unbundle(lib, tmp_path):
    """Every gfx950 code object inside the library `lib`, unbundled under tmp_path: [(path of the .co, text of its metadata notes)]."""
    fat = tmp_path / "fat.bin"
    subprocess.run([f"{LLVM_TOOLS}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", lib, str(tmp_path / "unused.so")], check=True)
    blob = fat.read_bytes()
    starts = [m.start() for m in re.finditer(b"__CLANG_OFFLOAD_BUNDLE__", blob)]
    assert starts, "no offload bundle in the library"
    out = []
    for k, at in enumerate(starts):
        piece = tmp_path / f"bundle{k}.bin"
        piece.write_bytes(blob[at:starts[k + 1] if k + 1 < len(starts) else len(blob)])
        co = tmp_path / f"bundle{k}.co"
        subprocess.run([f"{LLVM_TOOLS}/clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                        f"--input={piece}", f"--output={co}"], check=True)
        notes = subprocess.run([f"{LLVM_TOOLS}/llvm-readelf", "--notes", str(co)], check=True, capture_output=True, text=True).stdout
        out.append((co, notes))
    return out


@pytest.fixture(scope="module")
def code_objects(tmp_path_factory):
    """unbundle() of the library the tests load (a test module imports this fixture by name)."""
    if not have_llvm_tools():
        pytest.skip("LLVM binary tools not installed")
    return unbundle(os.path.join(ROOT, "sdf-viewer_amd", "libsdfgrid.so"), tmp_path_factory.mktemp("code_objects"))


def kernel_table(code_objects):
    """mangled name -> {vgpr, sgpr, vgpr_spill, sgpr_spill, lds, scratch, kernarg, co} from the code objects' metadata."""
    table = {}
    for co, notes in code_objects:
        for blk in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
            def field(key, blk=blk):
                return int(re.search(r"\." + key + r":\s+(\d+)", blk).group(1))
            name = re.search(r"\n\s+\.name:\s+(\S+)\n\s+\.private_segment_fixed_size", blk).group(1)
            table[name] = dict(vgpr=field("vgpr_count"), sgpr=field("sgpr_count"), vgpr_spill=field("vgpr_spill_count"),
                               sgpr_spill=field("sgpr_spill_count"), lds=field("group_segment_fixed_size"),
                               scratch=field("private_segment_fixed_size"), kernarg=field("kernarg_segment_size"), co=co)
    return table


def kernel_args(code_objects):
    """mangled name -> [(offset, size, value_kind), ...]: the explicit kernel arguments, in order, from the `.args` list of the
    code objects' metadata (the hidden_* entries the compiler appends are no part of a launch's argument array)."""
    table = {}
    for _, notes in code_objects:
        for blk in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
            name = re.search(r"\n\s+\.name:\s+(\S+)\n\s+\.private_segment_fixed_size", blk).group(1)
            listed = re.search(r"\n\s+\.args:\n(.*?)\n    \.\w+:", blk, re.S)
            args = []
            for entry in re.split(r"\n\s+- ", "\n" + listed.group(1))[1:] if listed else []:
                f = dict(re.findall(r"\.(\w+):\s+(\S+)", entry))
                if not f["value_kind"].startswith("hidden_"):
                    args.append((int(f["offset"]), int(f["size"]), f["value_kind"]))
            table[name] = args
    return table


def disassembly(co, symbol, cache={}):
    """The text of one kernel in llvm-objdump -d of its code object."""
    if co not in cache:
        text = subprocess.run([f"{LLVM_TOOLS}/llvm-objdump", "-d", str(co)], check=True, capture_output=True, text=True).stdout
        parts = re.split(r"\n[0-9a-f]{16} <([^>]+)>:\n", text)
        cache[co] = dict(zip(parts[1::2], parts[2::2]))
    return cache[co][symbol]


def opcodes(co, symbol):
    """The instruction stream of one kernel: ["opcode", "opcode nt", ...]."""
    ops = []
    for line in disassembly(co, symbol).split("\n"):
        code = line.split("//")[0].split()
        if code:
            ops.append(code[0] + (" nt" if "nt" in code[1:] else ""))
    return ops
