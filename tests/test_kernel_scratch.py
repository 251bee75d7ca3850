"""Private (scratch) memory of the chain kernels, read from the code-object notes of the built objects.

The two kernels ``bench.py`` runs -- the queue rounds ``mpp_deep_kernel<8,false,2,false,true,true,NCH>`` and the hot start
``mpp_chain_kernel<8,0,false,2,false,true>`` -- keep their whole live state in registers and LDS: no private segment, no
VGPR spill.  Every other instantiation of the two files may spill, but no more than it did before the round loop's
live state was cut down (the table below: bytes of scratch per lane at that commit).  Metadata only -- what
``profiles/tools/kernel_regs.sh`` prints; no instruction is looked at."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "mpp_cnn_rs_object_detection_amd", "csrc")

# scratch bytes per lane before this test existed.  mpp_deep_kernel: WAVES,DIAG,OCC,EXT,TAB,QUE
DEEP_BEFORE = {
    (1, 0, 1, 0, 0, 0): 0, (1, 0, 1, 0, 1, 0): 0, (1, 0, 1, 1, 0, 0): 9376, (1, 0, 2, 0, 0, 0): 68, (1, 0, 2, 0, 1, 0): 48,
    (1, 1, 1, 0, 0, 0): 0, (1, 1, 1, 0, 1, 0): 0, (1, 1, 1, 1, 0, 0): 9376, (1, 1, 2, 0, 0, 0): 140, (1, 1, 2, 0, 1, 0): 128,
    (2, 0, 1, 0, 0, 0): 0, (2, 0, 1, 0, 1, 0): 0, (2, 0, 2, 0, 0, 0): 72, (2, 0, 2, 0, 1, 0): 52,
    (2, 1, 1, 0, 0, 0): 0, (2, 1, 1, 0, 1, 0): 0, (2, 1, 2, 0, 0, 0): 152, (2, 1, 2, 0, 1, 0): 124,
    (4, 0, 1, 0, 0, 0): 0, (4, 0, 1, 0, 1, 0): 0, (4, 0, 2, 0, 0, 0): 168, (4, 0, 2, 0, 1, 0): 152,
    (4, 1, 1, 0, 0, 0): 0, (4, 1, 1, 0, 1, 0): 0, (4, 1, 2, 0, 0, 0): 248, (4, 1, 2, 0, 1, 0): 240,
    (8, 0, 2, 0, 0, 0): 164, (8, 0, 2, 0, 1, 0): 156, (8, 0, 2, 0, 1, 1): 152, (8, 0, 2, 1, 0, 0): 7568,
    (8, 1, 2, 0, 0, 0): 248, (8, 1, 2, 0, 1, 0): 240, (8, 1, 2, 0, 1, 1): 228, (8, 1, 2, 1, 0, 0): 7632,
}
# mpp_chain_kernel: WAVES,LPW,DIAG,OCC,SM,FAST
CHAIN_BEFORE = {
    (1, 0, 0, 1, 0, 0): 0, (1, 0, 0, 1, 0, 1): 0, (1, 0, 0, 1, 1, 0): 10624, (1, 0, 0, 2, 0, 0): 0, (1, 0, 0, 2, 0, 1): 0,
    (1, 0, 1, 1, 0, 0): 0, (1, 0, 1, 1, 1, 0): 10624,
    (16, 0, 0, 2, 0, 0): 648, (16, 0, 0, 4, 0, 0): 648, (16, 0, 1, 4, 0, 0): 704,
    (2, 0, 0, 1, 0, 0): 0, (2, 0, 0, 1, 0, 1): 0, (2, 0, 0, 2, 0, 0): 12, (2, 0, 0, 2, 0, 1): 0, (2, 0, 1, 1, 0, 0): 0,
    (4, 0, 0, 1, 0, 0): 0, (4, 0, 0, 1, 0, 1): 0, (4, 0, 0, 2, 0, 0): 60, (4, 0, 0, 2, 0, 1): 28, (4, 0, 1, 1, 0, 0): 0,
    (4, 1, 0, 1, 0, 0): 0, (4, 1, 0, 2, 0, 0): 56, (4, 1, 1, 1, 0, 0): 0,
    (4, 16, 0, 1, 0, 0): 0, (4, 16, 0, 2, 0, 0): 88, (4, 16, 1, 1, 0, 0): 0,
    (4, 2, 0, 1, 0, 0): 0, (4, 2, 0, 2, 0, 0): 88, (4, 2, 1, 1, 0, 0): 0,
    (4, 4, 0, 1, 0, 0): 0, (4, 4, 0, 2, 0, 0): 52, (4, 4, 1, 1, 0, 0): 0,
    (4, 8, 0, 1, 0, 0): 0, (4, 8, 0, 2, 0, 0): 88, (4, 8, 1, 1, 0, 0): 0,
    (8, 0, 0, 2, 0, 0): 60, (8, 0, 0, 2, 0, 1): 28, (8, 0, 0, 2, 1, 0): 8960, (8, 0, 1, 2, 0, 0): 100, (8, 0, 1, 2, 1, 0): 8992,
}
DEEP_PRODUCTION = (8, 0, 2, 0, 1, 1)          # the queue rounds, untraced (both chunk counts)
CHAIN_PRODUCTION = (8, 0, 0, 2, 0, 1)         # the hot start


def _tool(name):
    roots = [os.path.join(os.path.dirname(os.path.dirname(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))), "lib", "llvm", "bin"),
             os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")]
    for r in roots:
        p = os.path.join(r, name)
        if os.path.exists(p):
            return p
    return shutil.which(name)


def kernel_notes(obj, tmp_path):
    """{kernel name: {field: int}} of the gfx950 code object bundled in a host object file"""
    tools = {t: _tool(t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")}
    if not os.path.exists(obj) or not all(tools.values()):
        pytest.skip("needs the built objects (build()) and llvm-readelf")
    fat, dev = str(tmp_path / "fat.bin"), str(tmp_path / "dev.co")
    subprocess.check_call([tools["llvm-objcopy"], "-O", "binary", "--only-section=.hip_fatbin", obj, fat])
    subprocess.check_call([tools["clang-offload-bundler"], "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                           "--input=" + fat, "--output=" + dev, "--unbundle"])
    txt = subprocess.check_output([tools["llvm-readelf"], "--notes", dev], text=True)
    res = {}
    for blk in re.split(r"\n\s+- \.agpr_count", txt)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        if name:
            res[name.group(1)] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
                                  for k in ("private_segment_fixed_size", "vgpr_spill_count", "vgpr_count")}
    return res


def template_args(name, kernel):
    """the integer / bool template arguments of a mangled kernel name, in order"""
    m = re.match(r"_Z\d+%sI((?:L[ib]\d+E)+)E" % kernel, name)
    return tuple(int(v) for v in re.findall(r"L[ib](\d+)E", m.group(1))) if m else None


def test_deep_kernels_scratch(tmp_path):
    notes = kernel_notes(os.path.join(CSRC, "mpp_deep.o"), tmp_path)
    seen, production = set(), []
    for name, v in notes.items():
        args = template_args(name, "mpp_deep_kernel")
        if args is None:
            continue
        key, nch = args[:6], args[6]
        seen.add(key)
        assert key in DEEP_BEFORE, f"an instantiation without a row in the table: {args}"
        if key == DEEP_PRODUCTION:
            production.append(nch)
            assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0, (args, v)
        else:
            assert v["private_segment_fixed_size"] <= DEEP_BEFORE[key], (args, v, DEEP_BEFORE[key])
    assert seen == set(DEEP_BEFORE), set(DEEP_BEFORE) - seen
    assert sorted(production) == [2, 4]          # nmax <= 128 and nmax = 256


def test_chain_kernels_scratch(tmp_path):
    notes = kernel_notes(os.path.join(CSRC, "mpp_sampler.o"), tmp_path)
    seen = set()
    for name, v in notes.items():
        args = template_args(name, "mpp_chain_kernel")
        if args is None:
            continue
        seen.add(args)
        assert args in CHAIN_BEFORE, f"an instantiation without a row in the table: {args}"
        if args == CHAIN_PRODUCTION:
            assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0, (args, v)
        else:
            assert v["private_segment_fixed_size"] <= CHAIN_BEFORE[args], (args, v, CHAIN_BEFORE[args])
    assert seen == set(CHAIN_BEFORE), set(CHAIN_BEFORE) - seen
