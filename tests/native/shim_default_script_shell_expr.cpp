// tests/native/shim_default_script_shell_expr.cpp - VIAMD's default script plus two selections over SEVERAL within() shells behind the drop-in.
//
// `vn = sdf(s1, element('O') and within(6.0, resname("ALA")) and not within(3.5, resname("ALA")), 10.0);` is the spatial distribution of the
// SECOND hydration shell, and `nb = count(element('O') and within(3.5, residue(1:10)) and within(3.5, residue(11:20)));` the number of
// oxygens that bridge the two halves of the solute.  With all seven host opt-ins on (VMD_SCRIPT_FEATURE_ANGLES | _SHAPE |
// _RMSD | _WITHIN | _SHELL_RDF | _SHELL_SDF | _SHELL_EXPR) every property statement is the GPU's - d1, a1, r, v, lin, plan, iso, vn, nb -
// and the fallback is idle.  With a second argument "nobit" the host leaves VMD_SCRIPT_FEATURE_SHELL_EXPR off: vn and nb are reported with
// the reasons the one-term front-end gives, their statements stay in the fallback's text and the fallback is driven.  The host, the
// script, the common sequence (compile and split, drive, compare with a direct evaluation, interrupt, tear down) and the probes are
// shim_default_script_host.h's; this file holds the program's data and what is the expressions' own:
//   * vn is the GPU's: a 128^3 volume with voxels in it, voxelwise <= the static sdf of the same target list and different from it;
//     nb is a whole number per frame; vmd_eval_shell_mask names the members of a frame for both, and nb's row is its population
// Prints "OK frames=<F> properties=9 expr=gpu fallback_frame_range_calls=0 ..." (or "... expr=fallback ...") and exits 0.
#include "shim_default_script_host.h"

// md_mock_eval.h knows sdf( by its name but not count(): shim_mock_compile adds the property mdlib would have
static const ShimProgram kProgram = {
    "\nvn = sdf(s1, element('O') and within(6.0, resname(\"ALA\")) and not within(3.5, resname(\"ALA\")), 10.0);"
    "\nnb = count(element('O') and within(3.5, residue(1:10)) and within(3.5, residue(11:20)));",
    9, "count(", "nb", {{"vn", "vn = sdf(s1, element('O')"}, {"nb", "nb = count(element('O')"}, {"r", "rdf"}}};
static const char* kStaticScript = "s1 = resname(\"ALA\")[2:8];\nvn = sdf(s1, element('O'), 10.0);";
static const uint32_t kEarlier = VMD_SCRIPT_FEATURE_ANGLES | VMD_SCRIPT_FEATURE_SHAPE | VMD_SCRIPT_FEATURE_RMSD | VMD_SCRIPT_FEATURE_WITHIN | VMD_SCRIPT_FEATURE_SHELL_RDF | VMD_SCRIPT_FEATURE_SHELL_SDF;
static const ShimExpect kWithBit = {kEarlier | VMD_SCRIPT_FEATURE_SHELL_EXPR, {"d1", "a1", "r", "v", "lin", "plan", "iso", "vn", "nb"}, {}};
static const ShimExpect kNoBit = {kEarlier, {"d1", "a1", "r", "v", "lin", "plan", "iso"},
                                  {{"vn", "exactly one within() factor, found 2"}, {"nb", "count takes exactly one within() factor, found 2"}}};

int main(int argc, char** argv) {
    ShimHost h(ShimHost::frames_arg(argc, argv, 24));
    const bool shell_bit = !ShimHost::nobit_arg(argc, argv);
    const ShimExpect& want = shell_bit ? kWithBit : kNoBit;
    const size_t F = h.F;
    ShimRun run = shim_compile_and_split(h, kProgram, want);
    shim_create_and_drive(h, run, want);

    vmd_script_eval_t* e = shim_compare_with_direct(h, run.vir, run.ev, want.gpu_names);
    if (shell_bit) {
        shim_check_shell_sdf_against_static(h, e, "vn", kStaticScript);
        // the members of frame 1 by atom: water oxygens only, some of them
        const size_t members = shim_shell_members(h, e, "vn", 1, 1);
        if (members == 0 || members >= h.n_oxygen) fail("vmd_eval_shell_mask: some of the 953 oxygens");
        // nb: one whole number per frame, and the population vmd_eval_shell_mask reports for that frame
        const vmd_script_property_data_t* nb = vmd_eval_property_data(e, "nb");
        if (nb->dim[0] != (int32_t)F || nb->dim[1] != 1 || strcmp(nb->unit_str[1], "") != 0) fail("nb is the record of a within count");
        for (uint32_t f = 0; f < (uint32_t)std::min<size_t>(F, 3); ++f) {
            const size_t pop = shim_shell_members(h, e, "nb", 1, f);
            if ((float)pop != nb->values[f] || pop > h.n_oxygen) fail("nb's row is the population of its mask");
        }
        std::vector<uint64_t> words((h.N + 63) / 64);
        if (vmd_eval_shell_mask(e, "v", 1, &h.vsys, &h.vt, 1, words.data(), words.size()) != VMD_SHELL_MASK_FAILED) fail("a static sdf has no shell");
    }
    vmd_eval_free(e);
    // vn: voxels were counted; without the bit the record is the fallback's
    const double vn_voxels = shell_bit ? shim_shell_sdf_voxels(h, run.ev, "vn") : 0.0;
    shim_interrupt_and_restart(h, run, want);
    shim_tear_down(run);
    std::printf("OK frames=%zu properties=9 expr=%s fallback_frame_range_calls=%ld vn_voxels=%.0f\n", F, shell_bit ? "gpu" : "fallback",
                g_fallback_frame_range_calls.load(), vn_voxels);
    return 0;
}
