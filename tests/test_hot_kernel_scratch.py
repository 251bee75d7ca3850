"""Private (scratch) memory of the table form of the hot start, ``mpp_hot_kernel`` (csrc/mpp_hot.hip), read from the
code-object notes of the built object as tests/test_kernel_scratch.py reads them: like the hot start it replaces, the kernel
keeps its live state in registers and LDS -- no private segment, no VGPR spill.  Metadata only; no instruction is looked at."""
import os

from test_kernel_scratch import CSRC, kernel_notes


def test_hot_kernel_has_no_scratch(tmp_path):
    notes = kernel_notes(os.path.join(CSRC, "mpp_hot.o"), tmp_path)
    hot = {name: v for name, v in notes.items() if "mpp_hot_kernel" in name}
    assert len(hot) == 1, sorted(notes)                     # one instantiation: 8 waves, two per SIMD
    (name, v), = hot.items()
    assert name.startswith("_Z14mpp_hot_kernelILi8ELi2EE"), name
    assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0, v
    assert v["vgpr_count"] <= 256
