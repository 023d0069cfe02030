// tests/native/ir_replay.cpp - replays tests/golden/ir_cases.txt (the cases of tests/ir_cases.py, lists written out) through the vmd_ir_add_*
// entry points of viamd_amd/csrc/vmd_eval_ir.cpp, then asks every accepted descriptor list for its fingerprint, work estimate, flags and
// geometry atoms.  Built from this file and vmd_eval_ir.cpp alone, with -fsanitize=address,undefined, on the CPU: the sanitizers' report is
// the point (tests/test_ir_pin.py expects none); what it prints - per call `ok` or the refusal, per case the fingerprint - is compared with
// tests/golden/ir_pin.json.  The line format is described in tests/ir_cases.py.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <list>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "vmd_eval.h"

// what vmd_eval_ir.cpp takes from vmd_eval_runtime.cpp
thread_local std::string g_last_error;
bool vmd_fail(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return false;
}

struct Args {
    std::vector<std::string> w;
    size_t k = 0, last = 0;
    std::list<std::vector<int32_t>> lists;          // what the pointers handed out point into
    std::list<std::vector<uint32_t>> ulists;
    std::list<std::vector<uint8_t>> blists;
    std::list<std::string> strings;
    std::list<std::vector<const char*>> name_arrays;
    std::list<vmd_shell_t> shells;
    std::list<std::vector<vmd_shell_t>> shell_arrays;
    std::list<vmd_shell_expr_t> exprs;
    std::list<vmd_backbone_t> backbones;

    const std::string& word() { if (k >= w.size()) { fprintf(stderr, "line too short\n"); exit(2); } return w[k++]; }
    const char* name(const std::string& t) {
        if (t == "@null") return nullptr;
        strings.push_back(t == "@empty" ? "" : t);
        return strings.back().c_str();
    }
    const char* const* names() {
        const std::string t = word();
        if (t == "null") return nullptr;
        name_arrays.emplace_back();
        std::stringstream ss(t);
        std::string part;
        while (std::getline(ss, part, '/')) name_arrays.back().push_back(name(part));
        return name_arrays.back().data();
    }
    template <class T> const T* array(const std::string& t, std::list<std::vector<T>>& keep) {
        last = 0;
        if (t == "null") return nullptr;
        keep.emplace_back();
        std::stringstream ss(t);
        std::string part;
        while (std::getline(ss, part, ',')) keep.back().push_back((T)strtoll(part.c_str(), nullptr, 10));
        last = keep.back().size();
        return keep.back().data();
    }
    const int32_t* list() { return array(word(), lists); }
    size_t count(const std::string& t) { return t == "=" ? last : (size_t)strtoull(t.c_str(), nullptr, 10); }
    size_t count() { return count(word()); }
    float real(const std::string& t) { return strtof(t.c_str(), nullptr); }
    vmd_shell_t shell_struct(const std::string& t) {
        std::vector<std::string> f;
        std::stringstream ss(t);
        std::string part;
        while (std::getline(ss, part, ':')) f.push_back(part);
        vmd_shell_t h;
        h.ref = array(f[1], lists); h.nref = count(f[2]); h.rmin = real(f[3]); h.rmax = real(f[4]);
        return h;
    }
    const vmd_shell_t* shell() {
        const std::string t = word();
        if (t == "-") return nullptr;
        shells.push_back(shell_struct(t));
        return &shells.back();
    }
    const vmd_shell_expr_t* expr() {
        if (word() == "-") return nullptr;
        const std::string nterms = word();
        const uint32_t truth = (uint32_t)strtoul(word().c_str(), nullptr, 10);
        const size_t n = (size_t)strtoull(word().c_str(), nullptr, 10);
        shell_arrays.emplace_back();
        for (size_t i = 0; i < n; ++i) shell_arrays.back().push_back(shell_struct(word()));
        vmd_shell_expr_t x;
        x.terms = n ? shell_arrays.back().data() : nullptr;
        x.nterms = nterms == "=" ? n : (size_t)strtoull(nterms.c_str(), nullptr, 10);
        x.truth = truth;
        exprs.push_back(x);
        return &exprs.back();
    }
    const vmd_backbone_t* backbone() {
        if (word() == "-") return nullptr;
        const std::string nseg = word();
        vmd_backbone_t b;
        memset(&b, 0, sizeof(b));
        b.n = list();
        b.num_segments = count(nseg);
        b.ca = list(); b.c = list();
        b.num_ranges = (size_t)strtoull(word().c_str(), nullptr, 10);
        b.range_offsets = array(word(), ulists);
        b.rama_class = array(word(), blists);
        backbones.push_back(b);
        return &backbones.back();
    }
};

static bool call(vmd_script_ir_t* ir, const std::string& fn, Args& a) {
    // the arguments are read in the order of the entry point's signature (function arguments are evaluated in no fixed order: read first)
    if (fn == "rdf") { auto n = a.name(a.word()); auto r = a.list(); auto nr = a.count(); auto t = a.list(); auto nt = a.count();
        float lo = a.real(a.word()), hi = a.real(a.word()); return vmd_ir_add_rdf(ir, n, r, nr, t, nt, lo, hi); }
    if (fn == "sdf") { auto n = a.name(a.word()); auto s = a.list(); auto K = a.count(), m = a.count(); auto t = a.list(); auto nt = a.count();
        float c = a.real(a.word()); return vmd_ir_add_sdf(ir, n, s, K, m, t, nt, c); }
    if (fn == "distance") { auto n = a.name(a.word()); int kind = atoi(a.word().c_str()); auto x = a.list(); auto nx = a.count(); auto y = a.list();
        auto ny = a.count(); return vmd_ir_add_distance(ir, n, (vmd_distance_kind_t)kind, x, nx, y, ny); }
    if (fn == "distance_population") { auto n = a.name(a.word()); int kind = atoi(a.word().c_str()); auto P = a.count(); auto x = a.list();
        auto xo = a.list(); auto y = a.list(); auto yo = a.list(); return vmd_ir_add_distance_population(ir, n, (vmd_distance_kind_t)kind, P, x, xo, y, yo); }
    if (fn == "angle" || fn == "dihedral") {
        auto n = a.name(a.word());
        const int32_t* s[4] = {}; size_t c[4] = {};
        for (int k = 0; k < (fn == "angle" ? 3 : 4); ++k) { s[k] = a.list(); c[k] = a.count(); }
        return fn == "angle" ? vmd_ir_add_angle(ir, n, s[0], c[0], s[1], c[1], s[2], c[2])
                             : vmd_ir_add_dihedral(ir, n, s[0], c[0], s[1], c[1], s[2], c[2], s[3], c[3]);
    }
    if (fn == "angle_population" || fn == "dihedral_population") {
        auto n = a.name(a.word()); auto P = a.count();
        const int32_t* s[4] = {}; const int32_t* o[4] = {};
        for (int k = 0; k < (fn == "angle_population" ? 3 : 4); ++k) { s[k] = a.list(); o[k] = a.list(); }
        return fn == "angle_population" ? vmd_ir_add_angle_population(ir, n, P, s[0], o[0], s[1], o[1], s[2], o[2])
                                        : vmd_ir_add_dihedral_population(ir, n, P, s[0], o[0], s[1], o[1], s[2], o[2], s[3], o[3]);
    }
    if (fn == "shape_weights") { auto n = a.names(); auto x = a.list(); auto nx = a.count(); return vmd_ir_add_shape_weights(ir, n, x, nx); }
    if (fn == "shape_weights_population") { auto n = a.names(); auto P = a.count(); auto x = a.list(); auto o = a.list();
        return vmd_ir_add_shape_weights_population(ir, n, P, x, o); }
    if (fn == "rmsd") { auto n = a.name(a.word()); auto x = a.list(); auto nx = a.count(); return vmd_ir_add_rmsd(ir, n, x, nx); }
    if (fn == "rmsd_population") { auto n = a.name(a.word()); auto P = a.count(); auto x = a.list(); auto o = a.list();
        return vmd_ir_add_rmsd_population(ir, n, P, x, o); }
    if (fn == "within_count") { auto n = a.name(a.word()); auto t = a.list(); auto nt = a.count(); auto r = a.list(); auto nr = a.count();
        float lo = a.real(a.word()), hi = a.real(a.word()); return vmd_ir_add_within_count(ir, n, t, nt, r, nr, lo, hi); }
    if (fn == "rdf_shell") { auto n = a.name(a.word()); auto r = a.list(); auto nr = a.count(); auto rs = a.shell(); auto t = a.list(); auto nt = a.count();
        auto ts = a.shell(); float lo = a.real(a.word()), hi = a.real(a.word()); return vmd_ir_add_rdf_shell(ir, n, r, nr, rs, t, nt, ts, lo, hi); }
    if (fn == "sdf_shell") { auto n = a.name(a.word()); auto s = a.list(); auto K = a.count(), m = a.count(); auto t = a.list(); auto nt = a.count();
        auto ts = a.shell(); float c = a.real(a.word()); return vmd_ir_add_sdf_shell(ir, n, s, K, m, t, nt, ts, c); }
    if (fn == "within_count_expr") { auto n = a.name(a.word()); auto t = a.list(); auto nt = a.count(); auto x = a.expr();
        return vmd_ir_add_within_count_expr(ir, n, t, nt, x); }
    if (fn == "sdf_shell_expr") { auto n = a.name(a.word()); auto s = a.list(); auto K = a.count(), m = a.count(); auto t = a.list(); auto nt = a.count();
        auto x = a.expr(); float c = a.real(a.word()); return vmd_ir_add_sdf_shell_expr(ir, n, s, K, m, t, nt, x, c); }
    if (fn == "ramachandran") { auto n = a.names(); auto b = a.backbone(); return vmd_ir_add_ramachandran(ir, n, b); }
    fprintf(stderr, "unknown entry point %s\n", fn.c_str());
    exit(2);
}

// everything the pin asks of an accepted descriptor list, so that the sanitizers see those paths too
static void finish(vmd_script_ir_t* ir, long P) {
    if (!ir) return;
    const size_t n = vmd_ir_property_count(ir);
    const char* const* names = vmd_ir_property_names(ir);
    uint64_t sum = vmd_ir_work_per_frame(ir);
    std::vector<int32_t> buf(4096, -7);
    for (size_t i = 0; i < n; ++i) {
        sum += (uint64_t)vmd_ir_property_flags(ir, names[i]);
        for (long c : {-1L, 0L, P - 1, P}) {
            const size_t full = vmd_ir_geometry_atoms(ir, names[i], c, buf.data(), buf.size());
            std::vector<int32_t> half(full / 2 + 1, -7);                      // exactly the room that is offered, one guard entry behind it
            const size_t again = vmd_ir_geometry_atoms(ir, names[i], c, half.data(), full / 2);
            if (again != full || half[full / 2] != -7) { fprintf(stderr, "geometry_atoms: %s context %ld\n", names[i], c); exit(3); }
            sum += full;
        }
    }
    printf("= %llu %llu\n", (unsigned long long)vmd_ir_fingerprint(ir), (unsigned long long)sum);
    vmd_ir_free(ir);
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: ir_replay <ir_cases.txt>\n"); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    vmd_script_ir_t* ir = nullptr;
    long P = 1;
    std::string line;
    while (std::getline(in, line)) {
        std::stringstream ss(line);
        std::vector<std::string> w;
        std::string t;
        while (ss >> t) w.push_back(t);
        if (w.empty()) continue;
        if (w[0] == "case") {
            finish(ir, P);
            ir = vmd_ir_create();
            P = w.size() > 2 ? atol(w[2].c_str()) : 1;
            printf("case %s\n", w[1].c_str());
            continue;
        }
        Args a;
        a.w.assign(w.begin() + 2, w.end());
        g_last_error.clear();
        const bool ok = call(w[0] == "+" ? ir : nullptr, w[1], a);
        if (a.k != a.w.size()) { fprintf(stderr, "words left over: %s\n", line.c_str()); return 2; }
        printf("%s\n", ok ? "ok" : g_last_error.c_str());
    }
    finish(ir, P);
    return 0;
}
