// tests/native/shim_default_script_rmsd.cpp - VIAMD's default script plus `rm = rmsd(resname("ALA"));` behind the drop-in.
//
// The line is the one a user adds first when a protein is loaded.  With the three host opt-ins on (VMD_SCRIPT_FEATURE_ANGLES | _SHAPE |
// _RMSD) every property statement is the GPU's - d1, a1, r, v, lin, plan, iso, rm - and the fallback is idle.  With a second argument
// "nobit" the host leaves VMD_SCRIPT_FEATURE_RMSD off: `rm` is reported, its statement stays in the fallback's text, the mock evaluates it
// and the shim hands out the mock's values.  The host, the script and the common sequence (compile and split, drive, compare with a direct
// evaluation, interrupt, tear down) are shim_default_script_host.h's; this file holds the program's data and what is rmsd's own:
//   * rm is the GPU's: +0 at trajectory frame 0 (bit pattern), positive and finite later, in Angstrom; without the bit the mock's constant
//   * the MD_SCRIPT_VISUALIZE_ATOMS payload of rm marks the selection (the 200 atoms of the ALA residues)
// Prints "OK frames=<F> properties=8 rm=gpu ..." (or "... rm=fallback ...") and exits 0.
#include <cmath>

#include "shim_default_script_host.h"

// md_mock_eval.h does not know rmsd(): shim_mock_compile adds the property mdlib would have.  (No other rdf / sdf line: the bare names are gone too)
static const ShimProgram kProgram = {"\nrm = rmsd(resname(\"ALA\"));", 8, "rmsd(", "rm", {{"rm", "rm = rmsd(resname(\"ALA\"))"}, {"r", "rdf"}, {"v", "sdf"}}};
static const uint32_t kEarlier = VMD_SCRIPT_FEATURE_ANGLES | VMD_SCRIPT_FEATURE_SHAPE;
static const ShimExpect kWithBit = {kEarlier | VMD_SCRIPT_FEATURE_RMSD, {"d1", "a1", "r", "v", "lin", "plan", "iso", "rm"}, {}};
static const ShimExpect kNoBit = {kEarlier, {"d1", "a1", "r", "v", "lin", "plan", "iso"}, {{"rm", "'rmsd'"}}};

int main(int argc, char** argv) {
    ShimHost h(ShimHost::frames_arg(argc, argv, 24));
    const bool rmsd_bit = !ShimHost::nobit_arg(argc, argv);
    const ShimExpect& want = rmsd_bit ? kWithBit : kNoBit;
    const size_t F = h.F;
    ShimRun run = shim_compile_and_split(h, kProgram, want);
    shim_create_and_drive(h, run, want);

    vmd_script_eval_t* e = shim_compare_with_direct(h, run.vir, run.ev, want.gpu_names);
    if (rmsd_bit && strcmp(vmd_eval_property_data(e, "rm")->unit_str[1], "\xC3\x85") != 0) fail("rm is in Angstrom");
    vmd_eval_free(e);
    // rm: +0 at trajectory frame 0, a positive finite deviation later (the atoms jitter from frame to frame); without the bit the mock's constant
    double rm_max = 0.0;
    {
        const md_script_property_data_t* rm = shim_prop(run.ev, "rm");
        if (rm->dim[0] != (int32_t)F || rm->dim[1] != 1 || rm->num_values != F) fail("rm: one value per frame");
        for (size_t f = 0; f < F; ++f) {
            const float v = rm->values[f];
            if (!rmsd_bit) { if (v != MOCK_CPU_COPY) fail("without the bit rm is the fallback's"); continue; }
            uint32_t bits;
            memcpy(&bits, &v, 4);
            if (f == 0 && bits != 0u) fail("rm of trajectory frame 0 is +0, bit for bit");
            if (f > 0 && !(v > 0.0f && std::isfinite(v))) fail("rm of a later frame is positive and finite");
            rm_max = std::max(rm_max, (double)v);
        }
    }
    // the ATOMS payload of rm: the selection
    if (rmsd_bit && shim_count(shim_atoms_payload(h, run.eval_ir, "rm", -1)) != h.n_blob) fail("rm highlights the atoms of resname(\"ALA\")");
    shim_interrupt_and_restart(h, run, want);
    shim_tear_down(run);
    std::printf("OK frames=%zu properties=8 rm=%s fallback_frame_range_calls=%ld rm_max=%.3g\n", F, rmsd_bit ? "gpu" : "fallback",
                g_fallback_frame_range_calls.load(), rm_max);
    return 0;
}
