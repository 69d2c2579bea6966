"""What the gfx950 code object of a built translation unit says about a kernel's registers: the resource notes of
bayesian_dlms_amd/build/<object_name>, read without compiling anything (seconds).  The host tests of the kernel files assert their
bounds on what kernel_resources returns."""
import functools
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"


@functools.lru_cache(maxsize=None)
def _kernels(object_name):
    """{mangled kernel name: its block of the code object's metadata notes}; the object is built first when it is not there."""
    from bayesian_dlms_amd import build as b
    obj = os.path.join(ROOT, "bayesian_dlms_amd", "build", object_name)
    if not os.path.exists(obj):
        b.build()
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "gfx950.co")
        # (an output of its own: without one llvm-objcopy rewrites the object in place, and its new date hides a header edited since from build())
        subprocess.check_call([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", obj, os.path.join(tmp, "copy.o")])
        subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}",
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"])
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
    blocks = re.split(r"\n\s+- \.agpr_count:", notes)[1:]
    return {re.search(r"\.name:\s+(\S+)", blk).group(1): blk for blk in blocks}


def kernel_resources(object_name, kernel_substring):
    """(scratch bytes, spilled VGPRs, VGPRs) of the ONE kernel of the object whose mangled name contains kernel_substring."""
    kernels = _kernels(object_name)
    hit = [blk for name, blk in kernels.items() if kernel_substring in name]
    assert len(hit) == 1, (kernel_substring, sorted(kernels))
    get = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", hit[0]).group(1))
    return get("private_segment_fixed_size"), get("vgpr_spill_count"), get("vgpr_count")
