"""tools/isa_same.py --per-kernel: the cut of an assembly listing into per-kernel pieces (CPU, no compiler involved)."""
import os
import sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import isa_same  # noqa: E402


def listing(kernels, first_index=0):
    """A listing in the compiler's layout: per kernel a function, its descriptor, resource sets and info block; one metadata table."""
    text, meta = ["\t.amdgcn_target \"amdgcn-amd-amdhsa--gfx950\"", "\t.text"], ["\t.amdgpu_metadata", "---", "amdhsa.kernels:"]
    for k, (name, vgprs) in enumerate(kernels, first_index):
        text += [f"\t.protected\t{name} ; -- Begin function {name}", f"\t.type\t{name},@function", f"{name}:",
                 "\ts_load_dword s2, s[0:1], 0x0", f"\ts_cbranch_execz .LBB{k}_2", f".LBB{k}_1:{' ' * (30 - len(str(k)))}; =>This Loop Header: Depth=1",
                 "\tv_add_f32_e32 v0, v0, v1", f".LBB{k}_2:", "\ts_endpgm", "\t.section\t.rodata,\"a\",@progbits", f"\t.amdhsa_kernel {name}",
                 f"\t\t.amdhsa_next_free_vgpr {vgprs}", "\t.end_amdhsa_kernel", "\t.text", f".Lfunc_end{k}:",
                 f"\t.size\t{name}, .Lfunc_end{k}-{name}", f"\t.set {name}.num_vgpr, {vgprs}", "\t.section\t.AMDGPU.csdata,\"\",@progbits",
                 "; Kernel info:", f"; NumVgprs: {vgprs}", "\t.text"]
        meta += ["  - .agpr_count:     0", "    .args:", "      - .offset:         0", f"    .name:           {name}",
                 "    .sgpr_count:     10", f"    .vgpr_count:     {vgprs}"]
    return text + ["\t.section\t.AMDGPU.gpr_maximums,\"\",@progbits"] + meta + ["amdhsa.target:   amdgcn-amd-amdhsa--gfx950", "\t.end_amdgpu_metadata"]


def test_pieces_are_keyed_by_symbol_and_independent_of_the_function_index():
    a = isa_same.kernels(listing([("k_one", 8), ("k_two", 12)]))
    b = isa_same.kernels(listing([("k_other", 5)] * 11 + [("k_two", 12)]))          # k_two is function 11 of another file
    assert sorted(a) == ["k_one", "k_two"]
    assert a["k_two"] == b["k_two"] and a["k_one"] != a["k_two"]
    piece = "\n".join(a["k_two"])
    assert ".LBB_1: ; =>This Loop Header" in piece and ".Lfunc_end-k_two" in piece and "LBB1" not in piece
    assert ".amdhsa_kernel k_two" in piece and "; NumVgprs: 12" in piece          # descriptor and info block
    assert ".vgpr_count:     12" in piece and "k_one" not in piece                # its metadata entry, nobody else's
    assert "gpr_maximums" not in piece and "amdhsa.target" not in piece
    assert isa_same.counts(a["k_two"]) == {"AGPRs": 0, "SGPRs": 10, "VGPRs": 12, "instructions": 4}


def test_a_changed_register_count_or_instruction_shows(capsys):
    old, new = listing([("k_one", 8), ("k_two", 12)]), listing([("k_two", 12)])
    new2 = [ln.replace("v_add_f32_e32 v0, v0, v1", "v_add_f32_e32 v0, v1, v0") for ln in listing([("k_one", 8)])]
    assert isa_same.compare_kernels(["a.hip", "b.hip"], [old, new, None, new2], "REV") == 1
    out = capsys.readouterr().out
    assert "same       k_two  (a.hip," in out and "DIFFERENT  k_one  (a.hip -> b.hip," in out and "1 of 2 kernels" in out
    assert isa_same.compare_kernels(["a.hip"], [old, new], "REV") == 1
    assert "ONLY IN REV  k_one  (a.hip)" in capsys.readouterr().out
