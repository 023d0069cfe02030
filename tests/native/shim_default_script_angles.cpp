// tests/native/shim_default_script_angles.cpp - VIAMD's default script behind the drop-in with the host's angle opt-in on.
//
// The host compiles with VMD_SCRIPT_FEATURE_ANGLES: `a1 = angle(2,1,3) in resname("ALA")` joins d1 / r / v on the GPU and only
// `{lin,plan,iso} = shape_weights(all)` is left to mdlib.  The host, the script and the common sequence (compile and split, drive, compare
// with a direct evaluation, interrupt, tear down) are shim_default_script_host.h's; this file holds the program's data and what is the
// angle's own:
//   * a1 has one value per ALA residue and frame, in degrees, and agrees with the mock's own degree angle to 1e-4 deg
//   * lin / plan / iso are still the fallback's values
//   * the MD_SCRIPT_VISUALIZE_ATOMS payload of a1 marks atoms 2, 1 and 3 of every ALA residue (and of one residue for subidx >= 0)
// Prints "OK frames=<F> properties=7 a1=gpu ..." and exits 0.
#include <cmath>

#include "shim_default_script_host.h"

static const ShimProgram kProgram = {"", 7, nullptr, nullptr, {{"r", "rdf"}, {"v", "sdf"}}};     // (no other rdf / sdf line: the bare names are gone too)
// the fallback is not idle here: lin, plan and iso are its properties, so it walks every frame (shim_create_and_drive checks that it does)
static const ShimExpect kAngles = {VMD_SCRIPT_FEATURE_ANGLES, {"d1", "a1", "r", "v"}, {{"lin,plan,iso", nullptr}}};

int main(int argc, char** argv) {
    ShimHost h(ShimHost::frames_arg(argc, argv, 16));
    const size_t F = h.F, N = h.N, n_res = h.n_res;
    ShimRun run = shim_compile_and_split(h, kProgram, kAngles);
    shim_create_and_drive(h, run, kAngles);
    const md_script_property_data_t* a1 = shim_prop(run.ev, "a1");
    if (a1->dim[0] != (int32_t)F || a1->dim[1] != (int32_t)n_res) fail("a1: one value per ALA residue and frame");

    vmd_script_eval_t* e = shim_compare_with_direct(h, run.vir, run.ev, kAngles.gpu_names);
    if (strcmp(vmd_eval_property_data(e, "a1")->unit_str[1], "\xC2\xB0") != 0) fail("a1 is in degrees");
    vmd_eval_free(e);
    // ... and agrees with mdlib's (the mock's) degree angle wherever the residue's atoms are not split by the periodic faces (the mock
    // takes raw differences)
    size_t compared = 0;
    double worst = 0.0;
    {
        std::vector<float> x(N), y(N), z(N), row(n_res);
        const MockProp* ang = nullptr;
        for (const MockProp& p : run.eval_ir->props) if (p.kind == MockProp::ANGLE) ang = &p;
        if (!ang) fail("mock angle");
        for (size_t f = 0; f < F; ++f) {
            mock_load_frame(&h.mt, (int64_t)f, nullptr, x.data(), y.data(), z.data());
            mock_eval_row(*ang, x.data(), y.data(), z.data(), N, row.data());
            for (size_t c = 0; c < n_res; ++c) {
                const auto& ctx = ang->contexts[c];
                const int ia = ctx[(size_t)ang->i], ib = ctx[(size_t)ang->j], ic = ctx[(size_t)ang->k];
                bool whole = true;
                for (int q : {ia, ic}) whole = whole && std::fabs(x[q] - x[ib]) < 0.5f * h.L && std::fabs(y[q] - y[ib]) < 0.5f * h.L && std::fabs(z[q] - z[ib]) < 0.5f * h.L;
                if (!whole) continue;
                // the mock's fp32 acos loses digits as the angle nears 0 or 180 deg (d theta ~ 1 ulp / sin theta): 1e-4 deg there is the
                // mock's own error, not the backend's, so the bound widens with 1 / sin theta
                const double v = (double)a1->values[f * n_res + c], d = std::fabs(v - (double)row[c]);
                const double s = std::max(std::sin(v * M_PI / 180.0), 1e-3);
                if (getenv("SHIM_ANGLES_VERBOSE")) std::fprintf(stderr, "%zu %zu %.6f %.3g\n", f, c, v, d);
                worst = std::max(worst, d * std::min(1.0, s / 0.25));
                compared += 1;
            }
        }
        if (compared < F * n_res / 2) fail("too few whole residues to compare");
        if (worst > 1e-4) { std::fprintf(stderr, "worst %.3g deg\n", worst); fail("a1 differs from the mock's degree angle by more than 1e-4 deg"); }
    }
    // shape_weights is still mdlib's: the mock's own values
    {
        std::vector<float> x(N), y(N), z(N), row(4);
        mock_load_frame(&h.mt, 0, nullptr, x.data(), y.data(), z.data());
        for (const MockProp& p : run.eval_ir->props) {
            if (p.kind != MockProp::SHAPE) continue;
            mock_eval_row(p, x.data(), y.data(), z.data(), N, row.data());
            if (shim_prop(run.ev, p.name.c_str())->values[0] != row[0]) fail("lin / plan / iso are not the fallback's values");
        }
    }
    // the ATOMS payload of a1: atoms 2, 1, 3 (1-based, local) of each ALA residue
    {
        const auto ala = h.residues_of("ALA");
        const std::vector<char> all = shim_atoms_payload(h, run.eval_ir, "a1", -1);
        if (shim_count(all) != 3 * n_res) fail("a1 highlights three atoms per residue");
        for (const auto& r : ala) for (int k : {1, 0, 2}) if (!all[(size_t)r[(size_t)k]]) fail("a1 highlights atoms 2, 1, 3 of every ALA");
        const std::vector<char> one = shim_atoms_payload(h, run.eval_ir, "a1", 5);
        if (shim_count(one) != 3) fail("subidx selects one residue");
        for (int k : {1, 0, 2}) if (!one[(size_t)ala[5][(size_t)k]]) fail("subidx 5: atoms of the sixth ALA");
    }
    shim_interrupt_and_restart(h, run, kAngles);
    shim_tear_down(run);
    std::printf("OK frames=%zu properties=7 a1=gpu compared=%zu worst=%.3g\n", F, compared, worst);
    return 0;
}
