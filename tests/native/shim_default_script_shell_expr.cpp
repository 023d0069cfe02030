// tests/native/shim_default_script_shell_expr.cpp - VIAMD's default script plus two selections over SEVERAL within() shells behind the drop-in.
//
// `vn = sdf(s1, element('O') and within(6.0, resname("ALA")) and not within(3.5, resname("ALA")), 10.0);` is the spatial distribution of the
// SECOND hydration shell, and `nb = count(element('O') and within(3.5, residue(1:10)) and within(3.5, residue(11:20)));` the number of
// oxygens that bridge the two halves of the solute.  With all seven host opt-ins on (VMD_SCRIPT_FEATURE_ANGLES | _SHAPE |
// _RMSD | _WITHIN | _SHELL_RDF | _SHELL_SDF | _SHELL_EXPR) every property statement is the GPU's - d1, a1, r, v, lin, plan, iso, vn, nb -
// and the text left for mdlib (here the CPU mock of md_mock_eval.h behind VMD_SHIM_FALLBACK) holds the selection alone.  The program
// checks, through the md_* names:
//   * the backend compiles nine properties and reports nothing skipped; the fallback text keeps no property statement
//   * all nine come back through md_script_eval_property_data, bit-identical to direct vmd_* calls
//   * vn is the GPU's: a 128^3 volume with voxels in it, voxelwise <= the static sdf of the same target list and different from it;
//     nb is a whole number per frame; vmd_eval_shell_mask names the members of a frame for both, and nb's row is its population
//   * the fallback does no per-frame work: no call reaches its frame_range hook and the frame mask is complete
// Prints "OK frames=<F> properties=9 expr=gpu fallback_frame_range_calls=0 ..." and exits 0.
// With a second argument "nobit" the host leaves VMD_SCRIPT_FEATURE_SHELL_EXPR off: vn and nb are reported with the reasons the one-term
// front-end gives, their statements stay in the fallback's text and the fallback is driven: "OK frames=<F> properties=9 expr=fallback ...".
// md_mock_eval.h does not know count(); mock_compile() below adds the property mdlib would have to the mock's IR.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "md_mock.h"
#include "md_mock_eval.h"

// the fallback hooks: the mock's, with a counter in front of frame_range
static std::atomic<long> g_fallback_frame_range_calls{0};
#define countfb_md_script_eval_create mockmd_md_script_eval_create
#define countfb_md_script_eval_free mockmd_md_script_eval_free
#define countfb_md_script_eval_clear_data mockmd_md_script_eval_clear_data
#define countfb_md_script_eval_interrupt mockmd_md_script_eval_interrupt
#define countfb_md_script_eval_ir_fingerprint mockmd_md_script_eval_ir_fingerprint
#define countfb_md_script_eval_property_data mockmd_md_script_eval_property_data
#define countfb_md_script_eval_frame_mask mockmd_md_script_eval_frame_mask
#define countfb_md_script_ir_property_vis_payload mockmd_md_script_ir_property_vis_payload
#define countfb_md_script_vis_eval_payload mockmd_md_script_vis_eval_payload
static inline bool countfb_md_script_eval_frame_range(vmd_shim_fallback_eval_t* e, const md_script_ir_t* ir, const md_system_t* sys, md_trajectory_i* traj,
                                                      uint32_t frame_beg, uint32_t frame_end) {
    g_fallback_frame_range_calls += 1;
    return mockmd_md_script_eval_frame_range(e, ir, sys, traj, frame_beg, frame_end);
}
#define VMD_SHIM_FALLBACK(name) countfb_##name
#define VMD_SHIM_FALLBACK_DECLARED
#define VMD_SHIM_PREFIX(name) name
#include "vmd_md_script_shim.h"

// (md_mock_eval.h knows sdf( by its name; `nb = count(...)` is a temporal property of mdlib's IR, evaluated to MOCK_CPU_COPY like the others)
template <class ResiduesOf>
static md_script_ir_t* mock_compile(const char* source, ResiduesOf residues_of) {
    md_script_ir_t* ir = mock_ir_compile(source, residues_of);
    if (!ir || !strstr(source, "count(")) return ir;
    MockProp p;
    p.kind = MockProp::CPU_COPY; p.name = "nb"; p.flags = MD_SCRIPT_PROPERTY_FLAG_TEMPORAL;
    ir->props.push_back(p);
    ir->names.clear();
    for (auto& q : ir->props) ir->names.push_back(str_t{q.name.data(), q.name.size()});
    return ir;
}

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
    "s1 = resname(\"ALA\")[2:8];\nd1 = distance(10,30);\na1 = angle(2,1,3) in resname(\"ALA\");\nr = rdf(element('C'), element('H'), 10.0);\nv = sdf(s1, element('H'), 10.0);\n{lin,plan,iso} = shape_weights(all);\nvn = sdf(s1, element('O') and within(6.0, resname(\"ALA\")) and not within(3.5, resname(\"ALA\")), 10.0);\nnb = count(element('O') and within(3.5, residue(1:10)) and within(3.5, residue(11:20)));";
static const char* kStaticScript = "s1 = resname(\"ALA\")[2:8];\nvn = sdf(s1, element('O'), 10.0);";

int main(int argc, char** argv) {
    const size_t F = argc > 1 ? (size_t)std::atoi(argv[1]) : 24;
    const bool shell_bit = !(argc > 2 && !strcmp(argv[2], "nobit"));
    const size_t n_res = 20, n_blob = n_res * 10, N = n_blob + 933 * 3;
    const float L = 40.0f;
    if (vmd_device_count() <= 0) fail("no HIP device");
    vmd_shim_set_min_work(0);                     // this test system is far below the default threshold: send what is bound to the GPU

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

    md_script_ir_t* eval_ir = mock_compile(kDefaultScript, residues_of);
    if (!eval_ir || md_script_ir_property_count(eval_ir) != 9) fail("mock mdlib: the script has nine properties");
    // the opt-ins: the whole script is compiled for the GPU
    vmd_script_ir_t* vir = vmd_ir_create();
    vmd_script_report_t* report = nullptr;
    if (!vmd_ir_compile_from_source_ex(vir, kDefaultScript, &topo, VMD_SCRIPT_FEATURE_ANGLES | VMD_SCRIPT_FEATURE_SHAPE | VMD_SCRIPT_FEATURE_RMSD | VMD_SCRIPT_FEATURE_WITHIN | VMD_SCRIPT_FEATURE_SHELL_RDF | VMD_SCRIPT_FEATURE_SHELL_SDF | (shell_bit ? VMD_SCRIPT_FEATURE_SHELL_EXPR : 0u), &report)) fail("vmd_ir_compile_from_source_ex");
    const size_t n_gpu = shell_bit ? 9 : 7;
    if (vmd_ir_property_count(vir) != n_gpu || vmd_script_report_skipped_count(report) != 9 - n_gpu) fail("nine properties compiled and nothing skipped (without the bit: seven, vn and nb reported)");
    if (!shell_bit && (strcmp(vmd_script_report_skipped(report)[0].names, "vn") != 0 || !strstr(vmd_script_report_skipped(report)[0].reason, "exactly one within() factor, found 2") ||
                       strcmp(vmd_script_report_skipped(report)[1].names, "nb") != 0 || !strstr(vmd_script_report_skipped(report)[1].reason, "count takes exactly one within() factor, found 2")))
        fail("vn and nb are reported as ever");
    static const char* const want_names[9] = {"d1", "a1", "r", "v", "lin", "plan", "iso", "vn", "nb"};
    for (size_t i = 0; i < n_gpu; ++i) if (strcmp(vmd_ir_property_names(vir)[i], want_names[i]) != 0) fail("property order d1, a1, r, v, lin, plan, iso, vn, nb");
    const std::string reduced_text = vmd_script_report_fallback_source(report);
    vmd_script_report_free(report);
    if (reduced_text.size() != strlen(kDefaultScript)) fail("fallback source keeps the offsets of the editor's text");
    for (const char* gone : {"distance", "angle", "r = rdf", "v = sdf", "shape_weights", "lin"})
        if (reduced_text.find(gone) != std::string::npos) fail("the fallback text still holds a property statement");
    if ((reduced_text.find("vn = sdf(s1, element('O')") != std::string::npos) == shell_bit) fail("the sdf statement is the GPU's with the bit and the fallback's without it");
    if ((reduced_text.find("nb = count(element('O')") != std::string::npos) == shell_bit) fail("the count statement is the GPU's with the bit and the fallback's without it");
    if (reduced_text.find("s1 = resname(\"ALA\")[2:8];") != 0) fail("the fallback text keeps the selection");
    // what mdlib compiles from that text: no property at all
    md_script_ir_t* reduced = mock_compile(reduced_text.c_str(), residues_of);
    if (!reduced || md_script_ir_property_count(reduced) != 9 - n_gpu) fail("the reduced script holds no property (without the bit: vn and nb)");
    vmd_shim_bind_ir(eval_ir, vir);
    vmd_shim_bind_fallback_ir(eval_ir, reduced);
    md_allocator_i persistent{nullptr};

    md_script_eval_t* ev = md_script_eval_create(F, eval_ir, &persistent);
    if (!ev) fail("md_script_eval_create");
    if (!ev->fb || ev->fb->ir != reduced) fail("the fallback eval must be created from the reduced ir");
    if (md_script_eval_ir_fingerprint(ev) != md_script_ir_fingerprint(eval_ir)) fail("fingerprint: still the editor's script (src/main.cpp:987)");
    md_script_eval_clear_data(ev);
    for (uint32_t f = 0; f < (uint32_t)F; f += 3)
        if (!md_script_eval_frame_range(ev, eval_ir, &sys, sys.trajectory, f, std::min<uint32_t>(f + 3, (uint32_t)F))) fail("frame_range");
    if (!vmd_eval_wait_settled(ev->eval)) fail("settle");
    // no second evaluator walked the frames (without the bit it has to: vn and nb are its properties)
    if (shell_bit && g_fallback_frame_range_calls.load() != 0) fail("a call reached the fallback's frame_range although its ir holds no property");
    if (shell_bit && ev->fb->frames_evaluated.load() != 0) fail("the fallback evaluated frames");
    if (!shell_bit && g_fallback_frame_range_calls.load() == 0) fail("vn and nb stay with the fallback, which was not driven");
    const md_bitfield_t* fm = md_script_eval_frame_mask(ev);
    if (!fm) fail("frame mask");
    for (size_t f = 0; f < F; ++f) if (!md_bitfield_test_bit(fm, f)) fail("the frame mask is the GPU evaluator's alone: every frame done");

    const size_t num_props = md_script_ir_property_count(eval_ir);
    const str_t* prop_names = md_script_ir_property_names(eval_ir);
    for (size_t i = 0; i < num_props; ++i)
        if (!md_script_eval_property_data(ev, prop_names[i])) fail("a property of the default script disappeared behind the drop-in");
    auto prop = [&](const char* nm) { return md_script_eval_property_data(ev, str_t{nm, strlen(nm)}); };

    // all the compiled ones are the GPU's: bit-identical to a direct evaluation of the backend's IR
    {
        vmd_script_eval_t* e = vmd_eval_create(F, vir);
        vmd_system_t vsys = vmd_shim::wrap_system(&sys);
        vmd_trajectory_i vt = vmd_shim::wrap_trajectory(&traj_i);
        if (!e || !vmd_eval_frame_range(e, vir, &vsys, &vt, 0, (uint32_t)F) || !vmd_eval_wait_settled(e)) fail("direct evaluation");
        for (size_t i = 0; i < n_gpu; ++i) {
            const char* nm = want_names[i];
            const vmd_script_property_data_t* want = vmd_eval_property_data(e, nm);
            const md_script_property_data_t* got = prop(nm);
            if (!want || got->num_values != want->num_values || memcmp(got->values, want->values, want->num_values * sizeof(float)) != 0) fail("a property through the shim differs from direct vmd_* calls");
            for (size_t k = 0; k < got->num_values; ++k) if (got->values[k] == MOCK_CPU_COPY) fail("the shim handed out the fallback's copy of a bound property");
        }
        if (shell_bit) {
            const vmd_script_property_data_t* g = vmd_eval_property_data(e, "vn");
            if (g->dim[1] != VMD_VOLUME_DIM || g->dim[2] != VMD_VOLUME_DIM || g->dim[3] != VMD_VOLUME_DIM) fail("vn is an sdf record");
            // the static sdf of the same target list bounds it voxel by voxel, and is another volume
            vmd_script_ir_t* sir = vmd_ir_create();
            if (!vmd_ir_compile_from_source_ex(sir, kStaticScript, &topo, 0u, nullptr)) fail("static twin of vn");
            vmd_script_eval_t* se = vmd_eval_create(F, sir);
            if (!se || !vmd_eval_frame_range(se, sir, &vsys, &vt, 0, (uint32_t)F) || !vmd_eval_wait_settled(se)) fail("static twin: evaluation");
            const vmd_script_property_data_t* sg = vmd_eval_property_data(se, "vn");
            bool differs = false;
            for (size_t k = 0; k < g->num_values; ++k) { if (g->values[k] > sg->values[k]) fail("a voxel of the expression's sdf exceeds the static sdf's"); differs = differs || g->values[k] != sg->values[k]; }
            if (!differs) fail("the expression's sdf is the static sdf: the mask did nothing");
            vmd_eval_free(se);
            vmd_ir_free(sir);
            // the members of frame 1 by atom: water oxygens only, some of them, through the public product
            std::vector<uint64_t> words((N + 63) / 64);
            const size_t members = vmd_eval_shell_mask(e, "vn", 1, &vsys, &vt, 1, words.data(), words.size());
            if (members == VMD_SHELL_MASK_FAILED || members == 0 || members >= 953) fail("vmd_eval_shell_mask: some of the 953 oxygens");
            size_t bits = 0;
            for (size_t a = 0; a < N; ++a) if (words[a >> 6] >> (a & 63) & 1u) { bits += 1; if (strcmp(elements[a], "O") != 0) fail("a member that is not an oxygen"); }
            if (bits != members) fail("vmd_eval_shell_mask: the return value is the number of bits");
            if (vmd_eval_shell_mask(e, "vn", 1, &vsys, &vt, 1, words.data(), 1) != VMD_SHELL_MASK_FAILED) fail("cap too small must fail");
            // nb: one whole number per frame, and the population vmd_eval_shell_mask reports for that frame
            const vmd_script_property_data_t* nb = vmd_eval_property_data(e, "nb");
            if (nb->dim[0] != (int32_t)F || nb->dim[1] != 1 || strcmp(nb->unit_str[1], "") != 0) fail("nb is the record of a within count");
            for (uint32_t f = 0; f < (uint32_t)std::min<size_t>(F, 3); ++f) {
                const size_t pop = vmd_eval_shell_mask(e, "nb", 1, &vsys, &vt, f, words.data(), words.size());
                if (pop == VMD_SHELL_MASK_FAILED || (float)pop != nb->values[f] || pop > 953) fail("nb's row is the population of its mask");
            }
            if (vmd_eval_shell_mask(e, "v", 1, &vsys, &vt, 1, words.data(), words.size()) != VMD_SHELL_MASK_FAILED) fail("a static sdf has no shell");
        }
        vmd_eval_free(e);
    }
    // vn: voxels were counted; without the bit the record is the fallback's
    double gs_voxels = 0.0;
    {
        const md_script_property_data_t* gs = prop("vn");
        if (shell_bit) {
            const size_t nvox = (size_t)VMD_VOLUME_DIM * VMD_VOLUME_DIM * VMD_VOLUME_DIM;
            if (gs->dim[1] != VMD_VOLUME_DIM || gs->num_values != nvox) fail("vn: a volume of 128^3 voxels");
            for (size_t k = 0; k < gs->num_values; ++k) gs_voxels += gs->values[k];
            // at most one voxel per structure, frame and oxygen
            if (!(gs_voxels > 0.0) || !(gs_voxels < (double)F * 7.0 * 953.0)) fail("vn holds the voxels of the second shell");
        }
    }
    // interrupt / clear_data still reach both evaluators
    md_script_eval_interrupt(ev);
    if (ev->fb->interrupts.load() != 1) fail("interrupt was not forwarded to the fallback");
    md_script_eval_clear_data(ev);
    if (!md_script_eval_frame_range(ev, eval_ir, &sys, sys.trajectory, 0, 2)) fail("frame_range after interrupt + clear_data");
    if (shell_bit && g_fallback_frame_range_calls.load() != 0) fail("a call reached the fallback's frame_range after clear_data");
    md_script_eval_free(ev);
    vmd_shim_bind_fallback_ir(eval_ir, nullptr);
    vmd_shim_bind_ir(eval_ir, nullptr);
    vmd_ir_free(vir);
    md_script_ir_free(reduced);
    md_script_ir_free(eval_ir);
    std::printf("OK frames=%zu properties=9 expr=%s fallback_frame_range_calls=%ld vn_voxels=%.0f\n", F, shell_bit ? "gpu" : "fallback",
                g_fallback_frame_range_calls.load(), gs_voxels);
    return 0;
}
