// tests/native/shim_default_script_angles.cpp - VIAMD's default script behind the drop-in with the host's angle opt-in on.
//
// The host compiles with vmd_ir_compile_from_source_ex(..., VMD_SCRIPT_FEATURE_ANGLES, &report): `a1 = angle(2,1,3) in resname("ALA")`
// joins d1 / r / v on the GPU and only `{lin,plan,iso} = shape_weights(all)` is left to mdlib (here the CPU mock of md_mock_eval.h behind
// VMD_SHIM_FALLBACK).  The program checks, through the md_* names:
//   * the backend compiles d1, a1, r, v and reports lin,plan,iso alone; the fallback text keeps no angle statement
//   * all seven properties of mdlib's IR come back through md_script_eval_property_data
//   * a1 is the GPU evaluator's (bit-identical to direct vmd_* calls) and agrees with the mock's own degree angle to 1e-4 deg
//   * the MD_SCRIPT_VISUALIZE_ATOMS payload of a1 marks atoms 2, 1 and 3 of every ALA residue (and of one residue for subidx >= 0)
// Prints "OK frames=<F> properties=7 a1=gpu ..." and exits 0.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "md_mock.h"
#include "md_mock_eval.h"
#define VMD_SHIM_FALLBACK(name) mockmd_##name
#define VMD_SHIM_FALLBACK_DECLARED
#define VMD_SHIM_PREFIX(name) name
#include "vmd_md_script_shim.h"

static void fail(const char* what) {
    std::fprintf(stderr, "FAIL: %s (%s)\n", what, vmd_last_error());
    std::exit(1);
}

struct MockTraj { size_t F, N; float L; std::vector<float> xyz; };
static bool mock_get_header(void* inst, md_trajectory_header_t* h) { MockTraj* t = (MockTraj*)inst; h->num_frames = t->F; h->num_atoms = t->N; return true; }
static bool mock_load_frame(void* inst, int64_t idx, md_trajectory_frame_header_t* h, float* x, float* y, float* z) {
    MockTraj* t = (MockTraj*)inst;
    if (idx < 0 || (size_t)idx >= t->F) return false;
    const float* f = t->xyz.data() + (size_t)idx * 3 * t->N;
    if (x) memcpy(x, f, t->N * sizeof(float));
    if (y) memcpy(y, f + t->N, t->N * sizeof(float));
    if (z) memcpy(z, f + 2 * t->N, t->N * sizeof(float));
    if (h) { h->num_atoms = t->N; h->index = idx; h->timestamp = (double)idx; h->unitcell = md_unitcell_t{t->L, t->L, t->L, 0, 0, 0, 7u}; }
    return true;
}

// the literal of VIAMD's src/main.cpp:528
static const char* kDefaultScript =
    "s1 = resname(\"ALA\")[2:8];\nd1 = distance(10,30);\na1 = angle(2,1,3) in resname(\"ALA\");\nr = rdf(element('C'), element('H'), 10.0);\nv = sdf(s1, element('H'), 10.0);\n{lin,plan,iso} = shape_weights(all);";

int main(int argc, char** argv) {
    const size_t F = argc > 1 ? (size_t)std::atoi(argv[1]) : 16;
    const size_t n_res = 20, n_blob = n_res * 10, N = n_blob + 933 * 3;
    const float L = 40.0f;
    if (vmd_device_count() <= 0) fail("no HIP device");
    if (vmd_shim_min_work() != VMD_SHIM_MIN_WORK_DEFAULT) fail("default work threshold");
    vmd_shim_set_min_work(0);                     // this test system is far below the default threshold: send what is bound to the GPU (both sides: below)

    MockTraj mt{F, N, L, std::vector<float>(F * 3 * N)};
    {
        vmd_devtraj_t* dt = vmd_devtraj_create(F, N);
        if (!dt || !vmd_devtraj_synth(dt, 21, L, 0.05f, 0, 0, F)) fail("synth");
        vmd_trajectory_i* ti = vmd_devtraj_interface(dt);
        for (size_t f = 0; f < F; ++f) { float* p = mt.xyz.data() + f * 3 * N; if (!ti->load_frame(ti->inst, (int64_t)f, nullptr, p, p + N, p + 2 * N)) fail("download"); }
        vmd_devtraj_free(dt);
    }
    md_trajectory_i traj_i{&mt, mock_get_header, mock_load_frame};
    std::vector<float> sx(N), sy(N), sz(N), mass(N, 1.0f);
    md_system_t sys{};
    sys.atom.count = N; sys.atom.x = sx.data(); sys.atom.y = sy.data(); sys.atom.z = sz.data(); sys.atom.mass = mass.data();
    sys.unitcell = md_unitcell_t{L, L, L, 0, 0, 0, 7u};
    sys.trajectory = &traj_i;

    // the molecule's topology: 20 ALA residues of 10 atoms (N C C O C H H H C H), then waters - what selections resolve against
    static const char* ala[10] = {"N", "C", "C", "O", "C", "H", "H", "H", "C", "H"};
    std::vector<const char*> elements(N), resnames(N);
    std::vector<int32_t> residue_index(N);
    for (size_t i = 0; i < N; ++i) {
        if (i < n_blob) { elements[i] = ala[i % 10]; resnames[i] = "ALA"; residue_index[i] = (int32_t)(i / 10); }
        else { const size_t w = i - n_blob; elements[i] = w % 3 == 0 ? "O" : "H"; resnames[i] = "HOH"; residue_index[i] = (int32_t)(n_res + w / 3); }
    }
    vmd_topology_t topo{N, elements.data(), nullptr, resnames.data(), residue_index.data(), nullptr};
    auto residues_of = [&](const std::string& resname) {
        std::vector<std::vector<int32_t>> out;
        for (size_t i = 0; i < N; ++i) {
            if (resname != resnames[i]) continue;
            if (out.empty() || residue_index[(size_t)out.back().back()] != residue_index[i]) out.emplace_back();
            out.back().push_back((int32_t)i);
        }
        return out;
    };

    md_script_ir_t* eval_ir = mock_ir_compile(kDefaultScript, residues_of);
    if (!eval_ir || md_script_ir_property_count(eval_ir) != 7) fail("mock mdlib: the default script has seven properties");
    // the host's opt-in: the angle is compiled for the GPU too
    vmd_script_ir_t* vir = vmd_ir_create();
    vmd_script_report_t* report = nullptr;
    if (!vmd_ir_compile_from_source_ex(vir, kDefaultScript, &topo, VMD_SCRIPT_FEATURE_ANGLES, &report)) fail("vmd_ir_compile_from_source_ex");
    if (vmd_ir_property_count(vir) != 4 || vmd_script_report_skipped_count(report) != 1) fail("d1, a1, r, v compiled; {lin,plan,iso} reported");
    const char* const* names = vmd_ir_property_names(vir);
    if (strcmp(names[0], "d1") || strcmp(names[1], "a1") || strcmp(names[2], "r") || strcmp(names[3], "v")) fail("property order d1, a1, r, v");
    if (strcmp(vmd_script_report_skipped(report)[0].names, "lin,plan,iso") != 0) fail("skipped names");
    if (strstr(vmd_script_report_fallback_source(report), "angle") != nullptr) fail("the fallback text still holds the angle statement");
    vmd_script_report_free(report);
    vmd_shim_bind_ir(eval_ir, vir);
    md_allocator_i persistent{nullptr};

    md_script_eval_t* ev = md_script_eval_create(F, eval_ir, &persistent);
    if (!ev) fail("md_script_eval_create");
    const size_t num_props = md_script_ir_property_count(eval_ir);
    const str_t* prop_names = md_script_ir_property_names(eval_ir);
    md_script_eval_clear_data(ev);
    for (uint32_t f = 0; f < (uint32_t)F; f += 3)
        if (!md_script_eval_frame_range(ev, eval_ir, &sys, sys.trajectory, f, std::min<uint32_t>(f + 3, (uint32_t)F))) fail("frame_range");
    for (size_t i = 0; i < num_props; ++i)
        if (!md_script_eval_property_data(ev, prop_names[i])) fail("a property of the default script disappeared behind the drop-in");
    auto prop = [&](const char* nm) { return md_script_eval_property_data(ev, str_t{nm, strlen(nm)}); };
    const md_script_property_data_t* a1 = prop("a1");
    if (a1->dim[0] != (int32_t)F || a1->dim[1] != (int32_t)n_res) fail("a1: one value per ALA residue and frame");

    // a1 is the GPU's: bit-identical to a direct evaluation of the backend's IR
    {
        vmd_script_eval_t* e = vmd_eval_create(F, vir);
        vmd_system_t vsys = vmd_shim::wrap_system(&sys);
        vmd_trajectory_i vt = vmd_shim::wrap_trajectory(&traj_i);
        if (!e || !vmd_eval_frame_range(e, vir, &vsys, &vt, 0, (uint32_t)F) || !vmd_eval_wait_settled(e)) fail("direct evaluation");
        for (const char* nm : {"d1", "a1", "r", "v"}) {
            const vmd_script_property_data_t* want = vmd_eval_property_data(e, nm);
            const md_script_property_data_t* got = prop(nm);
            if (!want || got->num_values != want->num_values || memcmp(got->values, want->values, want->num_values * sizeof(float)) != 0) fail("d1 / a1 / r / v through the shim differ from direct vmd_* calls");
            for (size_t k = 0; k < got->num_values; ++k) if (got->values[k] == MOCK_CPU_COPY) fail("the shim handed out the fallback's copy of a bound property");
        }
        if (strcmp(vmd_eval_property_data(e, "a1")->unit_str[1], "\xC2\xB0") != 0) fail("a1 is in degrees");
        vmd_eval_free(e);
    }
    // ... and agrees with mdlib's (the mock's) degree angle wherever the residue's atoms are not split by the periodic faces (the mock
    // takes raw differences)
    size_t compared = 0;
    double worst = 0.0;
    {
        std::vector<float> x(N), y(N), z(N), row(n_res);
        const MockProp* ang = nullptr;
        for (const MockProp& p : eval_ir->props) if (p.kind == MockProp::ANGLE) ang = &p;
        if (!ang) fail("mock angle");
        for (size_t f = 0; f < F; ++f) {
            mock_load_frame(&mt, (int64_t)f, nullptr, x.data(), y.data(), z.data());
            mock_eval_row(*ang, x.data(), y.data(), z.data(), N, row.data());
            for (size_t c = 0; c < n_res; ++c) {
                const auto& ctx = ang->contexts[c];
                const int ia = ctx[(size_t)ang->i], ib = ctx[(size_t)ang->j], ic = ctx[(size_t)ang->k];
                bool whole = true;
                for (int q : {ia, ic}) whole = whole && std::fabs(x[q] - x[ib]) < 0.5f * L && std::fabs(y[q] - y[ib]) < 0.5f * L && std::fabs(z[q] - z[ib]) < 0.5f * L;
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
        mock_load_frame(&mt, 0, nullptr, x.data(), y.data(), z.data());
        for (const MockProp& p : eval_ir->props) {
            if (p.kind != MockProp::SHAPE) continue;
            mock_eval_row(p, x.data(), y.data(), z.data(), N, row.data());
            if (prop(p.name.c_str())->values[0] != row[0]) fail("lin / plan / iso are not the fallback's values");
        }
    }
    // the ATOMS payload of a1: atoms 2, 1, 3 (1-based, local) of each ALA residue
    {
        const auto ala = residues_of("ALA");
        md_allocator_i frame_alloc{nullptr};
        md_script_vis_ctx_t ctx = {eval_ir, &sys, sys.trajectory};
        const md_script_vis_payload_o* payload = md_script_ir_property_vis_payload(eval_ir, STR_LIT("a1"));
        if (!payload) fail("md_script_ir_property_vis_payload(a1)");
        md_script_vis_t vis = {};
        md_script_vis_init(&vis, &frame_alloc);
        if (!md_script_vis_eval_payload(&vis, payload, -1, &ctx, MD_SCRIPT_VISUALIZE_ATOMS)) fail("vis payload of a1");
        if (md_bitfield_popcount(&vis.atom_mask) != 3 * n_res) fail("a1 highlights three atoms per residue");
        for (const auto& r : ala) for (int k : {1, 0, 2}) if (!md_bitfield_test_bit(&vis.atom_mask, (uint64_t)r[(size_t)k])) fail("a1 highlights atoms 2, 1, 3 of every ALA");
        md_script_vis_free(&vis);
        md_script_vis_init(&vis, &frame_alloc);
        if (!md_script_vis_eval_payload(&vis, payload, 5, &ctx, MD_SCRIPT_VISUALIZE_ATOMS)) fail("vis payload of a1, one context");
        if (md_bitfield_popcount(&vis.atom_mask) != 3) fail("subidx selects one residue");
        for (int k : {1, 0, 2}) if (!md_bitfield_test_bit(&vis.atom_mask, (uint64_t)ala[5][(size_t)k])) fail("subidx 5: atoms of the sixth ALA");
        md_script_vis_free(&vis);
    }
    md_script_eval_free(ev);
    vmd_shim_bind_ir(eval_ir, nullptr);
    vmd_ir_free(vir);
    md_script_ir_free(eval_ir);
    std::printf("OK frames=%zu properties=7 a1=gpu compared=%zu worst=%.3g\n", F, compared, worst);
    return 0;
}
