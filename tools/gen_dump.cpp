// tools/gen_dump.cpp — what the kernel generator emits for an energy file, as text: every
// field of GenSource and the internal images generate() appended to the model, then the
// generated HIP source verbatim. Host-only (g++, no HIP runtime); two builds of the
// generator are compared by diffing their dumps (tools/gen_dump_matrix.sh, README).
//
//   gen_dump <energy.t> [--double] [--off32]      (OPT_AMD_GEN_* knobs from the environment)
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include "gen/codegen.h"

int main(int argc, char** argv) {
    const char* path = nullptr;
    bool dbl = false, off32 = false, bad = false;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--double")) dbl = true;
        else if (!strcmp(argv[i], "--off32")) off32 = true;
        else if (!path && argv[i][0] != '-') path = argv[i];
        else bad = true;
    }
    if (!path || bad) {
        fprintf(stderr, "usage: gen_dump <energy.t> [--double] [--off32]\n");
        return 2;
    }
    std::ifstream in(path);
    if (!in) {
        fprintf(stderr, "gen_dump: cannot read %s\n", path);
        return 2;
    }
    std::stringstream text;
    text << in.rdbuf();
    optamd::gen::GModel m;
    std::string err;
    if (!optamd::gen::build_model(text.str(), &m, &err)) {
        fprintf(stderr, "gen_dump: %s\n", err.c_str());
        return 1;
    }
    if (!m.unsupported.empty()) {
        fprintf(stderr, "gen_dump: unsupported: %s\n", m.unsupported.c_str());
        return 1;
    }
    const size_t declared = m.images.size();
    const optamd::gen::GenSource gs = optamd::gen::generate(m, dbl, off32);
    printf("// gen_dump: %s off32=%d\n", dbl ? "double" : "float", (int)off32);
    printf("// has_centered=%d has_graph=%d n_precompute=%d\n", (int)gs.has_centered, (int)gs.has_graph, gs.n_precompute);
    printf("// slot_base=%d,%d,%d,%d\n", gs.slot_base[0], gs.slot_base[1], gs.slot_base[2], gs.slot_base[3]);
    printf("// has_tiled=%d tiles=%dx%d tiled_lds=%zu instances_per_residual=%.17g prefer_tiled=%d\n", (int)gs.has_tiled,
           gs.tiles_x, gs.tiles_y, gs.tiled_lds, gs.instances_per_residual, (int)gs.prefer_tiled);
    printf("// has_strip=%d strip_cols=%d has_jtf_strip=%d jtf_strip_cols=%d has_cost_strip=%d cost_strip_cols=%d\n",
           (int)gs.has_strip, gs.strip_cols, (int)gs.has_jtf_strip, gs.jtf_strip_cols, (int)gs.has_cost_strip,
           gs.cost_strip_cols);
    printf("// graph_apply_centred=%d\n", (int)gs.graph_apply_centred);
    for (size_t i = 0; i < gs.dump.size(); ++i)
        printf("// dump[%zu]: graph=%d rows=%d nnz=%d\n", i, gs.dump[i].graph, gs.dump[i].rows, gs.dump[i].nnz);
    for (size_t i = 0; i < gs.nb_pairs.size(); ++i)
        printf("// nb_pairs[%zu]: %d %d\n", i, gs.nb_pairs[i].first, gs.nb_pairs[i].second);
    if (gs.has_dense) printf("// has_dense=1\n");   // LinearSolver("cholesky") (files without it print nothing here)
    // RobustEnergy statements (files without one print nothing here)
    for (size_t g = 0; g < m.loss.size(); ++g) {
        const optamd::gen::GLossGroup& L = m.loss[g];
        printf("// loss[%zu]: graph=%d kind=%s residuals=%zu scale=", g, L.graph, L.kind == L.Huber ? "huber" : "cauchy",
               L.residuals.size());
        if (L.scale_param >= 0) printf("param %d\n", L.scale_param);
        else printf("%.17g\n", L.scale);
    }
    for (size_t i = 0; i < gs.loss_inc.size(); ++i)
        printf("// loss_inc[%zu]: group=%d slot=%d\n", i, gs.loss_inc[i].first, gs.loss_inc[i].second);
    for (size_t i = declared; i < m.images.size(); ++i) {
        const optamd::gen::GImage& im = m.images[i];
        std::string dims;
        for (int d : im.dims) dims += (dims.empty() ? "" : ",") + std::to_string(d);
        printf("// image[%zu]: %s dims={%s} space=%d channels=%d elem=%s internal=%d tvalued=%d\n", i, im.name.c_str(),
               dims.c_str(), im.space, im.channels, im.elem.c_str(), (int)im.internal, (int)im.tvalued);
    }
    fputs(gs.code.c_str(), stdout);
    return 0;
}
