// tests/native/shim_default_script_host.h - TEST ONLY.  What the eight shim_default_script*.cpp programs share: the host of VIAMD's default
// script behind include/vmd_md_script_shim.h with the CPU mock of md_mock_eval.h as the evaluator behind it.
//   * the fallback hooks (the mock's, with a counter in front of frame_range), fail(), the mock trajectory, the default script's literal
//   * ShimHost: the synthetic 2 999-atom system (20 ALA residues of 10 atoms, 933 waters), its trajectory and topology for a frame count
//   * the sequence every opt-in program runs, as plain functions over a ShimRun, driven by the program's data (ShimProgram, ShimExpect):
//       shim_compile_and_split    mdlib (the mock) compiles the whole script, the backend what the feature bits allow; the report, the name
//                                 order, the fallback text and the IR mdlib compiles from it are checked; both IRs are bound
//       shim_create_and_drive     create, fingerprint, clear_data, frame_range in threes, settle; the fallback idle (or driven, when a
//                                 statement was left to it), the frame mask complete, every property of the script still there
//       shim_compare_with_direct  the backend's properties through the shim are bit-identical to a direct vmd_* evaluation
//       shim_interrupt_and_restart, shim_tear_down
//   * two probes several programs use: shim_atoms_payload (MD_SCRIPT_VISUALIZE_ATOMS), shim_shell_members (vmd_eval_shell_mask)
// A program keeps its data and the checks that are its feature's own.  shim_default_script.cpp (no opt-in: the fallback does real work and
// the masks are ANDed) has a flow of its own and uses the host, the trajectory and the probes only.
#pragma once
#include <algorithm>
#include <atomic>
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

[[noreturn]] static inline void fail(const char* what, const char* which = nullptr) {
    if (which) std::fprintf(stderr, "FAIL: %s [%s] (%s)\n", what, which, vmd_last_error());
    else std::fprintf(stderr, "FAIL: %s (%s)\n", what, vmd_last_error());
    std::exit(1);
}

struct MockTraj { size_t F, N; float L; std::vector<float> xyz; };
static inline bool mock_get_header(void* inst, md_trajectory_header_t* h) { MockTraj* t = (MockTraj*)inst; h->num_frames = t->F; h->num_atoms = t->N; return true; }
static inline bool mock_load_frame(void* inst, int64_t idx, md_trajectory_frame_header_t* h, float* x, float* y, float* z) {
    MockTraj* t = (MockTraj*)inst;
    if (idx < 0 || (size_t)idx >= t->F) return false;
    const float* f = t->xyz.data() + (size_t)idx * 3 * t->N;
    if (x) memcpy(x, f, t->N * sizeof(float));
    if (y) memcpy(y, f + t->N, t->N * sizeof(float));
    if (z) memcpy(z, f + 2 * t->N, t->N * sizeof(float));
    if (h) { h->num_atoms = t->N; h->index = idx; h->timestamp = (double)idx; h->unitcell = md_unitcell_t{t->L, t->L, t->L, 0, 0, 0, 7u}; }
    return true;
}

// the literal of VIAMD's src/main.cpp:528: six statements, seven properties.  A program appends its own line(s), each led by "\n"
static const char* const kDefaultScript =
    "s1 = resname(\"ALA\")[2:8];\nd1 = distance(10,30);\na1 = angle(2,1,3) in resname(\"ALA\");\nr = rdf(element('C'), element('H'), 10.0);\nv = sdf(s1, element('H'), 10.0);\n{lin,plan,iso} = shape_weights(all);";
static const char* const kDefaultSelection = "s1 = resname(\"ALA\")[2:8];";

// ---- the host: system, trajectory and topology for F frames ---------------------------------------------------------------------------
struct ShimHost {
    static constexpr size_t n_res = 20, n_blob = n_res * 10, n_water = 933, N = n_blob + n_water * 3, n_oxygen = n_res + n_water;
    static constexpr float L = 40.0f;
    const size_t F;
    MockTraj mt;
    md_trajectory_i traj_i;
    std::vector<float> sx, sy, sz, mass;
    md_system_t sys;
    std::vector<const char*> elements, resnames;    // the molecule's topology: what selections resolve against
    std::vector<int32_t> residue_index;
    vmd_topology_t topo;
    vmd_system_t vsys;                              // the same system and trajectory as a direct vmd_* caller hands them over
    vmd_trajectory_i vt;
    md_allocator_i persistent{nullptr};

    // <frames> of the command line, or the program's default
    static size_t frames_arg(int argc, char** argv, size_t dflt) { return argc > 1 ? (size_t)std::atoi(argv[1]) : dflt; }
    // [nobit]: the host leaves the program's newest feature bit off
    static bool nobit_arg(int argc, char** argv) { return argc > 2 && !strcmp(argv[2], "nobit"); }

    explicit ShimHost(size_t frames)
        : F(frames), mt{frames, N, L, std::vector<float>(frames * 3 * N)}, sx(N), sy(N), sz(N), mass(N, 1.0f), elements(N), resnames(N), residue_index(N) {
        if (vmd_device_count() <= 0) fail("no HIP device");
        if (vmd_shim_min_work() != VMD_SHIM_MIN_WORK_DEFAULT) fail("default work threshold");
        vmd_shim_set_min_work(0);                     // this test system is far below the default threshold: send what is bound to the GPU
        vmd_devtraj_t* dt = vmd_devtraj_create(F, N);
        if (!dt || !vmd_devtraj_synth(dt, 21, L, 0.05f, 0, 0, F)) fail("synth");
        vmd_trajectory_i* ti = vmd_devtraj_interface(dt);
        for (size_t f = 0; f < F; ++f) { float* p = mt.xyz.data() + f * 3 * N; if (!ti->load_frame(ti->inst, (int64_t)f, nullptr, p, p + N, p + 2 * N)) fail("download"); }
        vmd_devtraj_free(dt);
        traj_i = md_trajectory_i{&mt, mock_get_header, mock_load_frame};
        sys = md_system_t{};
        sys.atom.count = N; sys.atom.x = sx.data(); sys.atom.y = sy.data(); sys.atom.z = sz.data(); sys.atom.mass = mass.data();
        sys.unitcell = md_unitcell_t{L, L, L, 0, 0, 0, 7u};
        sys.trajectory = &traj_i;
        // 20 ALA residues of 10 atoms (N C C O C H H H C H), then waters
        static const char* ala[10] = {"N", "C", "C", "O", "C", "H", "H", "H", "C", "H"};
        for (size_t i = 0; i < N; ++i) {
            if (i < n_blob) { elements[i] = ala[i % 10]; resnames[i] = "ALA"; residue_index[i] = (int32_t)(i / 10); }
            else { const size_t w = i - n_blob; elements[i] = w % 3 == 0 ? "O" : "H"; resnames[i] = "HOH"; residue_index[i] = (int32_t)(n_res + w / 3); }
        }
        topo = vmd_topology_t{N, elements.data(), nullptr, resnames.data(), residue_index.data(), nullptr};
        vsys = vmd_shim::wrap_system(&sys);
        vt = vmd_shim::wrap_trajectory(&traj_i);
    }
    ShimHost(const ShimHost&) = delete;             // sys, topo, vsys and vt point into this object
    ShimHost& operator=(const ShimHost&) = delete;

    // the atoms of every residue of that name (what `in resname("ALA")` evaluates to)
    std::vector<std::vector<int32_t>> residues_of(const std::string& resname) const {
        std::vector<std::vector<int32_t>> out;
        for (size_t i = 0; i < N; ++i) {
            if (resname != resnames[i]) continue;
            if (out.empty() || residue_index[(size_t)out.back().back()] != residue_index[i]) out.emplace_back();
            out.back().push_back((int32_t)i);
        }
        return out;
    }
};

// mdlib's compiler: the mock's, plus the one statement md_mock_eval.h does not know (`function`, e.g. "rmsd("): its property `name` is a
// temporal property of mdlib's IR, evaluated by the mock to MOCK_CPU_COPY like the other hot-path properties
static inline md_script_ir_t* shim_mock_compile(const ShimHost& h, const char* source, const char* function = nullptr, const char* name = nullptr) {
    md_script_ir_t* ir = mock_ir_compile(source, [&h](const std::string& resname) { return h.residues_of(resname); });
    if (!ir || !function || !strstr(source, function)) return ir;
    MockProp p;
    p.kind = MockProp::CPU_COPY; p.name = name; p.flags = MD_SCRIPT_PROPERTY_FLAG_TEMPORAL;
    ir->props.push_back(p);
    ir->names.clear();
    for (auto& q : ir->props) ir->names.push_back(str_t{q.name.data(), q.name.size()});
    return ir;
}

static inline const md_script_property_data_t* shim_prop(const md_script_eval_t* e, const char* nm) { return md_script_eval_property_data(e, str_t{nm, strlen(nm)}); }

// ---- what an opt-in program says about itself ------------------------------------------------------------------------------------------
struct ShimStatement { const char* name; const char* text; };      // a property (the first of a tuple) and a piece of its statement's text
struct ShimSkipped { const char* names; const char* reason; };     // an entry of the skipped report: its names, a piece of its reason (or nullptr)
struct ShimExpect {                                                // one way to run the program: with its newest feature bit, or ("nobit") without
    uint32_t features;
    std::vector<const char*> gpu_names;                            // what the backend compiles, in order
    std::vector<ShimSkipped> skipped;                              // what it reports instead, in order: these statements stay mdlib's
    bool on_gpu(const char* name) const { for (const char* g : gpu_names) if (!strcmp(g, name)) return true; return false; }
};
struct ShimProgram {
    const char* extra_script;                                      // appended to kDefaultScript
    size_t num_properties;                                         // of mdlib's IR for the whole script
    const char* mock_function, *mock_name;                         // shim_mock_compile's addition, or nullptr
    std::vector<ShimStatement> statements;                         // the program's own lines; kDefaultStatements are checked for every program
};
// a statement's text is gone from the fallback's source when the backend took its property and is still there when it did not
static const ShimStatement kDefaultStatements[] = {{"d1", "distance"}, {"a1", "angle"}, {"r", "r = rdf"}, {"v", "v = sdf"}, {"lin", "shape_weights"}, {"lin", "lin"}};

struct ShimRun {
    std::string script;
    md_script_ir_t* eval_ir = nullptr;              // mdlib's IR of the whole script: what the host's md_* calls name
    vmd_script_ir_t* vir = nullptr;                 // the backend's IR
    md_script_ir_t* reduced = nullptr;              // mdlib's IR of the fallback text: what the evaluator behind the shim is given
    md_script_eval_t* ev = nullptr;
};

// the host's opt-in: compile with a report, check it, bind both IRs
static inline ShimRun shim_compile_and_split(const ShimHost& h, const ShimProgram& p, const ShimExpect& want) {
    ShimRun r;
    r.script = std::string(kDefaultScript) + p.extra_script;
    r.eval_ir = shim_mock_compile(h, r.script.c_str(), p.mock_function, p.mock_name);
    if (!r.eval_ir || md_script_ir_property_count(r.eval_ir) != p.num_properties) fail("mock mdlib: the number of properties of the script");
    r.vir = vmd_ir_create();
    vmd_script_report_t* report = nullptr;
    if (!vmd_ir_compile_from_source_ex(r.vir, r.script.c_str(), &h.topo, want.features, &report)) fail("vmd_ir_compile_from_source_ex");
    if (vmd_ir_property_count(r.vir) != want.gpu_names.size() || vmd_script_report_skipped_count(report) != want.skipped.size()) fail("the number of properties compiled and of statements reported");
    for (size_t i = 0; i < want.skipped.size(); ++i) {
        const vmd_script_skipped_t& s = vmd_script_report_skipped(report)[i];
        if (strcmp(s.names, want.skipped[i].names) != 0 || (want.skipped[i].reason && !strstr(s.reason, want.skipped[i].reason))) fail("a statement is not reported as ever", want.skipped[i].names);
    }
    for (size_t i = 0; i < want.gpu_names.size(); ++i) if (strcmp(vmd_ir_property_names(r.vir)[i], want.gpu_names[i]) != 0) fail("property order", want.gpu_names[i]);
    const std::string reduced_text = vmd_script_report_fallback_source(report);
    vmd_script_report_free(report);
    if (reduced_text.size() != r.script.size()) fail("fallback source keeps the offsets of the editor's text");
    auto check = [&](const ShimStatement& st) {
        const bool there = reduced_text.find(st.text) != std::string::npos;
        if (there && want.on_gpu(st.name)) fail("the fallback text still holds a statement the backend took", st.text);
        if (!there && !want.on_gpu(st.name)) fail("the fallback text lost a statement the backend left to mdlib", st.text);
    };
    for (const ShimStatement& st : kDefaultStatements) check(st);
    for (const ShimStatement& st : p.statements) check(st);
    if (reduced_text.find(kDefaultSelection) != 0) fail("the fallback text keeps the selection");
    // what mdlib compiles from that text: the reported properties alone
    r.reduced = shim_mock_compile(h, reduced_text.c_str(), p.mock_function, p.mock_name);
    if (!r.reduced || md_script_ir_property_count(r.reduced) != p.num_properties - want.gpu_names.size()) fail("the reduced script holds the reported properties alone");
    vmd_shim_bind_ir(r.eval_ir, r.vir);
    vmd_shim_bind_fallback_ir(r.eval_ir, r.reduced);
    return r;
}

// VIAMD's evaluation (src/main.cpp:966-997) in ranges of three frames, and what must hold when it has settled
static inline void shim_create_and_drive(ShimHost& h, ShimRun& r, const ShimExpect& want) {
    r.ev = md_script_eval_create(h.F, r.eval_ir, &h.persistent);
    if (!r.ev) fail("md_script_eval_create");
    if (!r.ev->fb || r.ev->fb->ir != r.reduced) fail("the fallback eval must be created from the reduced ir");
    if (md_script_eval_ir_fingerprint(r.ev) != md_script_ir_fingerprint(r.eval_ir)) fail("fingerprint: still the editor's script (src/main.cpp:987)");
    md_script_eval_clear_data(r.ev);
    for (uint32_t f = 0; f < (uint32_t)h.F; f += 3)
        if (!md_script_eval_frame_range(r.ev, r.eval_ir, &h.sys, h.sys.trajectory, f, std::min<uint32_t>(f + 3, (uint32_t)h.F))) fail("frame_range");
    if (!vmd_eval_wait_settled(r.ev->eval)) fail("settle");
    if (want.skipped.empty()) {                     // no second evaluator walked the frames
        if (g_fallback_frame_range_calls.load() != 0) fail("a call reached the fallback's frame_range although its ir holds no property");
        if (r.ev->fb->frames_evaluated.load() != 0) fail("the fallback evaluated frames");
    } else {                                        // it has to: the reported statements are its properties
        if (g_fallback_frame_range_calls.load() == 0) fail("a reported statement stays with the fallback, which was not driven", want.skipped[0].names);
        if (r.ev->fb->frames_evaluated.load() != (long)h.F) fail("the fallback did not evaluate every frame once");
    }
    const md_bitfield_t* fm = md_script_eval_frame_mask(r.ev);
    if (!fm) fail("frame mask");
    for (size_t f = 0; f < h.F; ++f) if (!md_bitfield_test_bit(fm, f)) fail("the frame mask: every frame done");
    const str_t* prop_names = md_script_ir_property_names(r.eval_ir);
    for (size_t i = 0; i < md_script_ir_property_count(r.eval_ir); ++i)
        if (!md_script_eval_property_data(r.ev, prop_names[i])) fail("a property of the default script disappeared behind the drop-in");
}

// `names` through the shim (`ev`) are the GPU's: bit-identical to a direct evaluation of the backend's IR, never the fallback's CPU copy.
// Returns the direct eval for the program's own look at its records; the program frees it (vmd_eval_free)
static inline vmd_script_eval_t* shim_compare_with_direct(ShimHost& h, const vmd_script_ir_t* vir, const md_script_eval_t* ev, const std::vector<const char*>& names) {
    vmd_script_eval_t* e = vmd_eval_create(h.F, vir);
    if (!e || !vmd_eval_frame_range(e, vir, &h.vsys, &h.vt, 0, (uint32_t)h.F) || !vmd_eval_wait_settled(e)) fail("direct evaluation");
    for (const char* nm : names) {
        const vmd_script_property_data_t* want = vmd_eval_property_data(e, nm);
        const md_script_property_data_t* got = shim_prop(ev, nm);
        if (!want || got->num_values != want->num_values || memcmp(got->values, want->values, want->num_values * sizeof(float)) != 0) fail("a property through the shim differs from direct vmd_* calls", nm);
        for (size_t k = 0; k < got->num_values; ++k) if (got->values[k] == MOCK_CPU_COPY) fail("the shim handed out the fallback's copy of a bound property", nm);
    }
    return e;
}

// interrupt / clear_data still reach both evaluators, and the eval runs again
static inline void shim_interrupt_and_restart(ShimHost& h, ShimRun& r, const ShimExpect& want) {
    md_script_eval_interrupt(r.ev);
    if (r.ev->fb->interrupts.load() != 1) fail("interrupt was not forwarded to the fallback");
    md_script_eval_clear_data(r.ev);
    if (!md_script_eval_frame_range(r.ev, r.eval_ir, &h.sys, h.sys.trajectory, 0, 2)) fail("frame_range after interrupt + clear_data");
    if (want.skipped.empty() && g_fallback_frame_range_calls.load() != 0) fail("a call reached the fallback's frame_range after clear_data");
}

static inline void shim_tear_down(ShimRun& r) {
    md_script_eval_free(r.ev);
    if (g_mock_live_evals.load() != 0) fail("md_script_eval_free must free the fallback evals too");
    vmd_shim_bind_fallback_ir(r.eval_ir, nullptr);
    vmd_shim_bind_ir(r.eval_ir, nullptr);
    vmd_ir_free(r.vir);
    md_script_ir_free(r.reduced);
    md_script_ir_free(r.eval_ir);
}

// ---- probes ---------------------------------------------------------------------------------------------------------------------------
// the atoms the MD_SCRIPT_VISUALIZE_ATOMS payload of a property marks (all contexts: subidx -1), one flag per atom
static inline std::vector<char> shim_atoms_payload(ShimHost& h, const md_script_ir_t* ir, const char* name, int subidx) {
    md_allocator_i frame_alloc{nullptr};
    md_script_vis_ctx_t ctx = {ir, &h.sys, h.sys.trajectory};
    const md_script_vis_payload_o* payload = md_script_ir_property_vis_payload(ir, str_t{name, strlen(name)});
    if (!payload) fail("md_script_ir_property_vis_payload", name);
    md_script_vis_t vis = {};
    md_script_vis_init(&vis, &frame_alloc);
    if (!md_script_vis_eval_payload(&vis, payload, subidx, &ctx, MD_SCRIPT_VISUALIZE_ATOMS)) fail("vis payload", name);
    std::vector<char> atoms(h.N);
    for (size_t a = 0; a < h.N; ++a) atoms[a] = md_bitfield_test_bit(&vis.atom_mask, a);
    md_script_vis_free(&vis);
    return atoms;
}
static inline size_t shim_count(const std::vector<char>& atoms) { return (size_t)std::count(atoms.begin(), atoms.end(), (char)1); }

// the members of a within() shell of `name` at one frame through the public product (vmd_eval_shell_mask on a direct eval): the return value
// is the number of bits, every member is an oxygen (every shell of these scripts is `element('O') and ...`), a cap too small fails.
// (The scripts of shim_default_script.cpp, _angles, _shape and _rmsd hold no within(): they have no shell to ask for.)
static inline size_t shim_shell_members(ShimHost& h, vmd_script_eval_t* e, const char* name, int which, uint32_t frame) {
    std::vector<uint64_t> words((h.N + 63) / 64);
    const size_t members = vmd_eval_shell_mask(e, name, which, &h.vsys, &h.vt, frame, words.data(), words.size());
    if (members == VMD_SHELL_MASK_FAILED) fail("vmd_eval_shell_mask", name);
    size_t bits = 0;
    for (size_t a = 0; a < h.N; ++a) if (words[a >> 6] >> (a & 63) & 1u) { bits += 1; if (strcmp(h.elements[a], "O") != 0) fail("a member that is not an oxygen", name); }
    if (bits != members) fail("vmd_eval_shell_mask: the return value is the number of bits", name);
    if (vmd_eval_shell_mask(e, name, which, &h.vsys, &h.vt, frame, words.data(), 1) != VMD_SHELL_MASK_FAILED) fail("cap too small must fail", name);
    return members;
}

// the sdf over a shell `name` of a direct eval is a 128^3 volume that the static sdf of the same target list (`static_script`, same name)
// bounds voxel by voxel, and another volume
static inline void shim_check_shell_sdf_against_static(ShimHost& h, vmd_script_eval_t* e, const char* name, const char* static_script) {
    const vmd_script_property_data_t* g = vmd_eval_property_data(e, name);
    if (g->dim[1] != VMD_VOLUME_DIM || g->dim[2] != VMD_VOLUME_DIM || g->dim[3] != VMD_VOLUME_DIM) fail("not an sdf record", name);
    vmd_script_ir_t* sir = vmd_ir_create();
    if (!vmd_ir_compile_from_source_ex(sir, static_script, &h.topo, 0u, nullptr)) fail("static twin", name);
    vmd_script_eval_t* se = vmd_eval_create(h.F, sir);
    if (!se || !vmd_eval_frame_range(se, sir, &h.vsys, &h.vt, 0, (uint32_t)h.F) || !vmd_eval_wait_settled(se)) fail("static twin: evaluation");
    const vmd_script_property_data_t* sg = vmd_eval_property_data(se, name);
    bool differs = false;
    for (size_t k = 0; k < g->num_values; ++k) { if (g->values[k] > sg->values[k]) fail("a voxel of the shell's sdf exceeds the static sdf's", name); differs = differs || g->values[k] != sg->values[k]; }
    if (!differs) fail("the shell's sdf is the static sdf: the mask did nothing", name);
    vmd_eval_free(se);
    vmd_ir_free(sir);
}

// the sum of the sdf `name` through the shim: a 128^3 volume with voxels in it, at most one per structure (7), frame and oxygen
static inline double shim_shell_sdf_voxels(const ShimHost& h, const md_script_eval_t* ev, const char* name) {
    const md_script_property_data_t* gs = shim_prop(ev, name);
    const size_t nvox = (size_t)VMD_VOLUME_DIM * VMD_VOLUME_DIM * VMD_VOLUME_DIM;
    if (gs->dim[1] != VMD_VOLUME_DIM || gs->num_values != nvox) fail("not a volume of 128^3 voxels", name);
    double voxels = 0.0;
    for (size_t k = 0; k < gs->num_values; ++k) voxels += gs->values[k];
    if (!(voxels > 0.0) || !(voxels < (double)h.F * 7.0 * (double)h.n_oxygen)) fail("the volume does not hold the voxels of the shell", name);
    return voxels;
}
