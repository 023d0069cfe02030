// tests/native/shim_default_script_shape.cpp - VIAMD's default script behind the drop-in with BOTH host opt-ins on.
//
// The host compiles with VMD_SCRIPT_FEATURE_ANGLES | VMD_SCRIPT_FEATURE_SHAPE: every property statement of the script is the GPU's - d1,
// a1, r, v, lin, plan, iso - and the text left for mdlib holds the selection `s1 = ...;` alone, so the fallback is idle.  The host, the
// script and the common sequence (compile and split, drive, compare with a direct evaluation, interrupt, tear down) are
// shim_default_script_host.h's; this file holds the program's data and what is shape_weights' own:
//   * lin / plan / iso are the GPU's: Westin's measures (each in [0, 1], summing to 1, no unit), not the mock's sorted coordinate variances
//   * the MD_SCRIPT_VISUALIZE_ATOMS payload of lin marks the selection (all atoms)
// Prints "OK frames=<F> properties=7 a1=gpu lin=gpu ..." and exits 0.
#include <cmath>

#include "shim_default_script_host.h"

static const ShimProgram kProgram = {"", 7, nullptr, nullptr, {{"r", "rdf"}, {"v", "sdf"}}};     // (no other rdf / sdf line: the bare names are gone too)
static const ShimExpect kBoth = {VMD_SCRIPT_FEATURE_ANGLES | VMD_SCRIPT_FEATURE_SHAPE, {"d1", "a1", "r", "v", "lin", "plan", "iso"}, {}};

int main(int argc, char** argv) {
    ShimHost h(ShimHost::frames_arg(argc, argv, 24));
    const size_t F = h.F, N = h.N;
    ShimRun run = shim_compile_and_split(h, kProgram, kBoth);
    shim_create_and_drive(h, run, kBoth);

    vmd_script_eval_t* e = shim_compare_with_direct(h, run.vir, run.ev, kBoth.gpu_names);
    if (strcmp(vmd_eval_property_data(e, "lin")->unit_str[1], "") != 0) fail("lin has no unit");
    vmd_eval_free(e);
    // lin / plan / iso: Westin's measures of the covariance matrix, not the mock's formula
    double worst_sum = 0.0;
    size_t differ = 0;
    {
        const md_script_property_data_t* w[3] = {shim_prop(run.ev, "lin"), shim_prop(run.ev, "plan"), shim_prop(run.ev, "iso")};
        std::vector<float> x(N), y(N), z(N);
        for (int k = 0; k < 3; ++k) if (w[k]->dim[0] != (int32_t)F || w[k]->dim[1] != 1 || w[k]->num_values != F) fail("lin / plan / iso: one value per frame");
        for (size_t f = 0; f < F; ++f) {
            double sum = 0.0;
            for (int k = 0; k < 3; ++k) { const float v = w[k]->values[f]; if (!(v >= 0.0f && v <= 1.0f)) fail("a weight outside [0, 1]"); sum += (double)v; }
            worst_sum = std::max(worst_sum, std::fabs(sum - 1.0));
            float mock[3];
            mock_load_frame(&h.mt, (int64_t)f, nullptr, x.data(), y.data(), z.data());
            mock_shape(x.data(), y.data(), z.data(), N, mock);
            for (int k = 0; k < 3; ++k) differ += w[k]->values[f] != mock[k];
        }
        if (worst_sum > 3e-7) fail("lin + plan + iso != 1");
        if (differ == 0) fail("lin / plan / iso are the mock's values");
    }
    // the ATOMS payload of lin: the selection
    if (shim_count(shim_atoms_payload(h, run.eval_ir, "lin", -1)) != N) fail("lin highlights every atom of `all`");
    shim_interrupt_and_restart(h, run, kBoth);
    shim_tear_down(run);
    std::printf("OK frames=%zu properties=7 a1=gpu lin=gpu fallback_frame_range_calls=0 sum_error=%.3g\n", F, worst_sum);
    return 0;
}
