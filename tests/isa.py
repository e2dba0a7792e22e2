"""What the ISA tests share: a translation unit cross-compiled to gfx950 assembly (no GPU needed) and the code-object
metadata read off it."""
import os
import re
import shutil
import subprocess

from visgeom_amd import _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hipcc():
    return shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


def device_asm(compiler, unit, out):
    """the device assembly of csrc/<unit>, compiled with the library's flags, as text"""
    flags = [f for f in _build.HIPCC_FLAGS if f != "-shared"]
    cmd = [compiler] + flags + ["--cuda-device-only", "-S", "-I", os.path.join(ROOT, "include"),
                                os.path.join(_build.CSRC, unit), "-o", out]
    subprocess.run(cmd, check=True, capture_output=True)
    return open(out).read()


def kernel_metadata(text):
    """kernel name -> {field: value} of the code object metadata (.vgpr_count, .private_segment_fixed_size, ...)"""
    meta = text[text.find("amdhsa.kernels:"):]
    out = {}
    for entry in re.split(r"\n  - (?=\.)", meta)[1:]:
        fields = dict(re.findall(r"^\s*-?\s*(\.[a-z_]+):\s+(\S+)$", "    " + entry, flags=re.M))
        if ".name" in fields:
            out[fields[".name"]] = fields
    return out
