"""CPU check of the shipped code objects: libdvccorr.so carries the fp32 convc1-fused on-the-fly kernel
(k_fused_proj_f32<R, KS>, csrc/fused_proj_f32.hip) for every radius 1..4 and channel step count KS in {1, 2, 4},
and none of those instances spills: the kernel is laid out for one wave per SIMD (the split query operands take
192 VGPRs at C_pad 128), and a scratch spill inside its MFMA loop would undo that."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

LIB = os.path.join(ROOT, "raft-dvc_amd", "dvccorr", "libdvccorr.so")


def _instances():
    import isa_check
    assert os.path.exists(LIB), "libdvccorr.so missing: run __graft_entry__.build()"
    out = {}
    for name, res in isa_check.kernel_resources(LIB).items():
        m = re.search(r"k_fused_proj_f32ILi(\d)ELi(\d)E", name)
        if m:
            out[(int(m.group(1)), int(m.group(2)))] = res
    return out


def test_library_has_every_instance():
    inst = _instances()
    assert sorted(inst) == [(r, ks) for r in (1, 2, 3, 4) for ks in (1, 2, 4)], sorted(inst)


def test_instances_do_not_spill():
    inst = _instances()
    assert inst, "no k_fused_proj_f32 instance in libdvccorr.so"
    bad = {k: (v.get(".vgpr_spill_count"), v.get(".sgpr_spill_count"), v.get(".private_segment_fixed_size"))
           for k, v in inst.items()
           if v.get(".vgpr_spill_count", 0) or v.get(".sgpr_spill_count", 0) or v.get(".private_segment_fixed_size", 0)}
    assert not bad, f"(R, KS): (vgpr spills, sgpr spills, scratch bytes) {bad}"
    assert all(v.get(".group_segment_fixed_size", 0) <= 160 * 1024 for v in inst.values())
