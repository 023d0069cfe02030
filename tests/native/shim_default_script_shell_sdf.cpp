// tests/native/shim_default_script_shell_sdf.cpp - VIAMD's default script plus an sdf over a hydration shell behind the drop-in.
//
// `gs = sdf(s1, element('O') and within(3.5, resname("ALA")), 10.0);` is the spatial distribution of the water in contact with the
// solute, not of all water inside the cube.  With all six host opt-ins on (VMD_SCRIPT_FEATURE_ANGLES | _SHAPE | _RMSD |
// _WITHIN | _SHELL_RDF | _SHELL_SDF) every property statement is the GPU's - d1, a1, r, v, lin, plan, iso, gs - and the fallback is idle.
// With a second argument "nobit" the host leaves VMD_SCRIPT_FEATURE_SHELL_SDF off: `gs` is reported ("unsupported function 'within'"),
// its statement stays in the fallback's text and the fallback is driven.  The host, the script, the common sequence (compile and split,
// drive, compare with a direct evaluation, interrupt, tear down) and the probes are shim_default_script_host.h's; this file holds the
// program's data and what is the shell sdf's own:
//   * gs is the GPU's: a 128^3 volume with voxels in it, voxelwise <= the static sdf of the same target list and different from it;
//     vmd_eval_shell_mask names its members of a frame, and refuses the static sdf v
// Prints "OK frames=<F> properties=8 gs=gpu ..." (or "... gs=fallback ...") and exits 0.
#include "shim_default_script_host.h"

// (md_mock_eval.h knows sdf( by its name: the line is a volume of the mock's IR, evaluated to MOCK_CPU_COPY like the others)
static const ShimProgram kProgram = {"\ngs = sdf(s1, element('O') and within(3.5, resname(\"ALA\")), 10.0);", 8, nullptr, nullptr, {{"gs", "gs = sdf(s1, element('O')"}, {"r", "rdf"}}};
static const char* kStaticScript = "s1 = resname(\"ALA\")[2:8];\ngs = sdf(s1, element('O'), 10.0);";
static const uint32_t kEarlier = VMD_SCRIPT_FEATURE_ANGLES | VMD_SCRIPT_FEATURE_SHAPE | VMD_SCRIPT_FEATURE_RMSD | VMD_SCRIPT_FEATURE_WITHIN | VMD_SCRIPT_FEATURE_SHELL_RDF;
static const ShimExpect kWithBit = {kEarlier | VMD_SCRIPT_FEATURE_SHELL_SDF, {"d1", "a1", "r", "v", "lin", "plan", "iso", "gs"}, {}};
static const ShimExpect kNoBit = {kEarlier, {"d1", "a1", "r", "v", "lin", "plan", "iso"}, {{"gs", "'within'"}}};

int main(int argc, char** argv) {
    ShimHost h(ShimHost::frames_arg(argc, argv, 24));
    const bool shell_bit = !ShimHost::nobit_arg(argc, argv);
    const ShimExpect& want = shell_bit ? kWithBit : kNoBit;
    ShimRun run = shim_compile_and_split(h, kProgram, want);
    shim_create_and_drive(h, run, want);

    vmd_script_eval_t* e = shim_compare_with_direct(h, run.vir, run.ev, want.gpu_names);
    if (shell_bit) {
        shim_check_shell_sdf_against_static(h, e, "gs", kStaticScript);
        // the members of frame 1 by atom: water oxygens only, some of them
        const size_t members = shim_shell_members(h, e, "gs", 1, 1);
        if (members == 0 || members >= h.n_oxygen) fail("vmd_eval_shell_mask: some of the 953 oxygens");
        std::vector<uint64_t> words((h.N + 63) / 64);
        if (vmd_eval_shell_mask(e, "v", 1, &h.vsys, &h.vt, 1, words.data(), words.size()) != VMD_SHELL_MASK_FAILED) fail("a static sdf has no shell");
    }
    vmd_eval_free(e);
    // gs: voxels were counted; without the bit the record is the fallback's
    const double gs_voxels = shell_bit ? shim_shell_sdf_voxels(h, run.ev, "gs") : 0.0;
    shim_interrupt_and_restart(h, run, want);
    shim_tear_down(run);
    std::printf("OK frames=%zu properties=8 gs=%s fallback_frame_range_calls=%ld gs_voxels=%.0f\n", h.F, shell_bit ? "gpu" : "fallback",
                g_fallback_frame_range_calls.load(), gs_voxels);
    return 0;
}
