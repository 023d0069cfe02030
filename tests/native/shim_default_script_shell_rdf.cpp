// tests/native/shim_default_script_shell_rdf.cpp - VIAMD's default script plus an rdf over a hydration shell behind the drop-in.
//
// `gs = rdf(element('O') and within(3.5, resname("ALA")), element('O'), 8.0);` is the structure of the water around the first shell of
// a solute.  With the host opt-ins on (VMD_SCRIPT_FEATURE_ANGLES | _SHAPE | _SHELL_RDF) every property statement is the
// GPU's - d1, a1, r, v, lin, plan, iso, gs - and the fallback is idle.  With a second argument "nobit" the host leaves
// VMD_SCRIPT_FEATURE_SHELL_RDF off: `gs` is reported ("unsupported function 'within'"), its statement stays in the fallback's text and the
// fallback is driven.  The host, the script and the common sequence (compile and split, drive, compare with a direct evaluation,
// interrupt, tear down) are shim_default_script_host.h's; this file holds the program's data and what is the shell rdf's own:
//   * gs is the GPU's: a distribution of 1 024 bins with pairs in it and no unit; vmd_eval_shell_mask names the members of its reference side
// Prints "OK frames=<F> properties=8 gs=gpu ..." (or "... gs=fallback ...") and exits 0.
#include "shim_default_script_host.h"

// (md_mock_eval.h knows rdf( by its name: the line is a distribution of the mock's IR, evaluated to MOCK_CPU_COPY like the others)
static const ShimProgram kProgram = {"\ngs = rdf(element('O') and within(3.5, resname(\"ALA\")), element('O'), 8.0);", 8, nullptr, nullptr, {{"gs", "gs = rdf(element('O')"}, {"v", "sdf"}}};
static const uint32_t kEarlier = VMD_SCRIPT_FEATURE_ANGLES | VMD_SCRIPT_FEATURE_SHAPE;
static const ShimExpect kWithBit = {kEarlier | VMD_SCRIPT_FEATURE_SHELL_RDF, {"d1", "a1", "r", "v", "lin", "plan", "iso", "gs"}, {}};
static const ShimExpect kNoBit = {kEarlier, {"d1", "a1", "r", "v", "lin", "plan", "iso"}, {{"gs", "'within'"}}};

int main(int argc, char** argv) {
    ShimHost h(ShimHost::frames_arg(argc, argv, 24));
    const bool shell_bit = !ShimHost::nobit_arg(argc, argv);
    const ShimExpect& want = shell_bit ? kWithBit : kNoBit;
    const size_t F = h.F;
    ShimRun run = shim_compile_and_split(h, kProgram, want);
    shim_create_and_drive(h, run, want);

    vmd_script_eval_t* e = shim_compare_with_direct(h, run.vir, run.ev, want.gpu_names);
    if (shell_bit) {
        const vmd_script_property_data_t* g = vmd_eval_property_data(e, "gs");
        if (g->dim[2] != VMD_RDF_NUM_BINS || strcmp(g->unit_str[1], "") != 0 || !g->counts || !g->weights64) fail("gs is an rdf record");
        // the members of frame 1 by atom: the shell is the reference side; the target side is a static set
        const size_t members = shim_shell_members(h, e, "gs", 0, 1);
        if (members == 0 || members >= h.n_oxygen) fail("vmd_eval_shell_mask: some of the 953 oxygens");
        std::vector<uint64_t> words((h.N + 63) / 64);
        if (vmd_eval_shell_mask(e, "gs", 1, &h.vsys, &h.vt, 1, words.data(), words.size()) != VMD_SHELL_MASK_FAILED) fail("a static side has no shell");
    }
    vmd_eval_free(e);
    // gs: pairs were counted and weighted; without the bit the record is the fallback's
    double gs_pairs = 0.0, gs_weight = 0.0;
    if (shell_bit) {
        const md_script_property_data_t* gs = shim_prop(run.ev, "gs");
        if (gs->dim[2] != VMD_RDF_NUM_BINS || gs->num_values != VMD_RDF_NUM_BINS || !gs->weights) fail("gs: a distribution of 1 024 bins");
        for (size_t k = 0; k < gs->num_values; ++k) { gs_pairs += gs->values[k]; gs_weight += gs->weights[k]; }
        // at least the pairs among the 20 oxygens of the ALA residues and their first shell; far fewer than all O-O pairs
        if (!(gs_pairs > 0.0) || !(gs_weight > 0.0) || !(gs_pairs < (double)F * 953.0 * 953.0)) fail("gs holds the pairs of the shell");
    }
    shim_interrupt_and_restart(h, run, want);
    shim_tear_down(run);
    std::printf("OK frames=%zu properties=8 gs=%s fallback_frame_range_calls=%ld gs_pairs=%.0f\n", F, shell_bit ? "gpu" : "fallback",
                g_fallback_frame_range_calls.load(), gs_pairs);
    return 0;
}
