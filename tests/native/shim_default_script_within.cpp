// tests/native/shim_default_script_within.cpp - VIAMD's default script plus a hydration-number line behind the drop-in.
//
// `nw = count(element('O') and within(3.5, resname("ALA")));` is the dynamic selection people write first: the population of a shell
// around a solute, per frame.  With the host opt-ins on (VMD_SCRIPT_FEATURE_ANGLES | _SHAPE | _WITHIN) every property statement is the
// GPU's - d1, a1, r, v, lin, plan, iso, nw - and the fallback is idle.  With a second argument "nobit" the host leaves
// VMD_SCRIPT_FEATURE_WITHIN off: `nw` is reported, its statement stays in the fallback's text, the mock evaluates it and the shim hands out
// the mock's values.  The host, the script and the common sequence (compile and split, drive, compare with a direct evaluation, interrupt,
// tear down) are shim_default_script_host.h's; this file holds the program's data and what is the count's own:
//   * nw is the GPU's: a whole number per frame, at least the 20 oxygens of the ALA residues themselves (D-WITHIN-SELF), at most the
//     953 oxygens of the system, no unit, the population vmd_eval_shell_mask reports; without the bit the mock's constant
//   * the MD_SCRIPT_VISUALIZE_ATOMS payload of nw marks the static candidates: the reference set and the target set
// Prints "OK frames=<F> properties=8 nw=gpu ..." (or "... nw=fallback ...") and exits 0.
#include <cmath>

#include "shim_default_script_host.h"

// md_mock_eval.h does not know count(): shim_mock_compile adds the property mdlib would have.  (No other rdf / sdf line: the bare names are gone too)
static const ShimProgram kProgram = {"\nnw = count(element('O') and within(3.5, resname(\"ALA\")));", 8, "count(", "nw", {{"nw", "nw = count(element('O')"}, {"r", "rdf"}, {"v", "sdf"}}};
static const uint32_t kEarlier = VMD_SCRIPT_FEATURE_ANGLES | VMD_SCRIPT_FEATURE_SHAPE;
static const ShimExpect kWithBit = {kEarlier | VMD_SCRIPT_FEATURE_WITHIN, {"d1", "a1", "r", "v", "lin", "plan", "iso", "nw"}, {}};
static const ShimExpect kNoBit = {kEarlier, {"d1", "a1", "r", "v", "lin", "plan", "iso"}, {{"nw", "'count'"}}};

int main(int argc, char** argv) {
    ShimHost h(ShimHost::frames_arg(argc, argv, 24));
    const bool within_bit = !ShimHost::nobit_arg(argc, argv);
    const ShimExpect& want = within_bit ? kWithBit : kNoBit;
    const size_t F = h.F;
    ShimRun run = shim_compile_and_split(h, kProgram, want);
    shim_create_and_drive(h, run, want);

    vmd_script_eval_t* e = shim_compare_with_direct(h, run.vir, run.ev, want.gpu_names);
    if (within_bit) {
        const vmd_script_property_data_t* nw = vmd_eval_property_data(e, "nw");
        if (strcmp(nw->unit_str[1], "") != 0) fail("nw has no unit");
        for (uint32_t f = 0; f < (uint32_t)std::min<size_t>(F, 3); ++f)
            if ((float)shim_shell_members(h, e, "nw", 1, f) != nw->values[f]) fail("nw's row is the population of its mask");
    }
    vmd_eval_free(e);
    // nw: a whole number per frame between the 20 oxygens of the ALA residues (each within 0 of itself) and all 953 oxygens; without the
    // bit the mock's constant
    double nw_min = 1e30, nw_max = 0.0;
    {
        const md_script_property_data_t* nw = shim_prop(run.ev, "nw");
        if (nw->dim[0] != (int32_t)F || nw->dim[1] != 1 || nw->num_values != F) fail("nw: one value per frame");
        for (size_t f = 0; f < F; ++f) {
            const float v = nw->values[f];
            if (!within_bit) { if (v != MOCK_CPU_COPY) fail("without the bit nw is the fallback's"); continue; }
            if (!(v >= (float)h.n_res && v <= (float)h.n_oxygen) || v != std::floor(v)) fail("nw is a whole number in [20, 953]");
            nw_min = std::min(nw_min, (double)v); nw_max = std::max(nw_max, (double)v);
        }
    }
    // the ATOMS payload of nw: the static candidates - the 200 atoms of the ALA residues and the 953 oxygens, 20 of them in both
    if (within_bit && shim_count(shim_atoms_payload(h, run.eval_ir, "nw", -1)) != h.n_blob + h.n_water) fail("nw highlights the reference set and the target set");
    shim_interrupt_and_restart(h, run, want);
    shim_tear_down(run);
    std::printf("OK frames=%zu properties=8 nw=%s fallback_frame_range_calls=%ld nw_min=%.0f nw_max=%.0f\n", F, within_bit ? "gpu" : "fallback",
                g_fallback_frame_range_calls.load(), within_bit ? nw_min : 0.0, nw_max);
    return 0;
}
