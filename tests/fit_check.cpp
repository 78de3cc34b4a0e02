// fit_check.cpp -- the host layer of the device-side verifier fit as a plain host program: openwakeword_amd/csrc/owwhip_fit_host.h alone,
// no HIP, built with -fsanitize=address,undefined by tests/test_verifier_fit_cpu.py, which holds the output to the Python restatement
// (tests/verifier_fit_ref.py: slab_plan, tile_map) and to the refusals the header documents.
//   fit_check FILE     one case per line of FILE:  name T C budget on_device pool_cap pool_used labels U off_0 .. off_U
//                      labels: alt (window i has label i & 1), ones, bad (a 2 at the last window); the first pool_used slots are taken
// Per case: "case NAME rc R" (R < 0: refused, with "err TEXT"), then "prob u status id n_pos n_neg x_off" per problem, "slab first
// last rows k_floats tiles" per slab and "tile slab p tr tc" per tile (only the first 64 of a slab, plus "tiles slab count").
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "owwhip_fit_host.h"

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: fit_check FILE\n"); return 2; }
    std::ifstream in(argv[1]);
    std::string line;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        std::istringstream ls(line);
        std::string name, labels_mode, c_text;                        // (C as text: "nan" must get through)
        int T, on_device, pool_cap, pool_used, U;
        long long budget;
        ls >> name >> T >> c_text >> budget >> on_device >> pool_cap >> pool_used >> labels_mode >> U;
        const float C = strtof(c_text.c_str(), nullptr);
        std::vector<int64_t> off((size_t)std::max(U, 0) + 1);
        for (auto& o : off) ls >> o;
        if (!ls) { fprintf(stderr, "fit_check: bad line '%s'\n", line.c_str()); return 2; }
        const long long n = off.back() > 0 ? off.back() : 0;
        uint8_t* labels = (uint8_t*)malloc((size_t)n + 1);           // (exactly the windows of the call, + 1 so that n = 0 has an address)
        for (long long i = 0; i < n; ++i) labels[i] = labels_mode == "ones" ? 1 : (uint8_t)(i & 1);
        if (labels_mode == "bad" && n > 0) labels[n - 1] = 2;
        std::vector<int> pool_T((size_t)pool_cap, 0);
        for (int v = 0; v < pool_used; ++v) pool_T[v] = 16;
        std::vector<oww_fit_result> res((size_t)std::max(U, 1));
        const int TR = 34;
        const float dummy = 0.f;                                      // the windows are never read by the host layer
        int rc = owf::check_args(true, pool_cap, &dummy, off.data(), labels, U, T, TR, C, res.data());
        if (rc == 0 && U > 0) {
            owf::classify(off.data(), labels, U, res.data());
            rc = owf::assign_ids(pool_T, U, res.data());
        }
        printf("case %s rc %d\n", name.c_str(), rc);
        if (rc < 0) { printf("err %s\n", owp::g_err.c_str()); free(labels); continue; }
        const long long D = (long long)T * OWW_EMB_DIM;
        std::vector<int> run, Ns;
        for (int u = 0; u < U; ++u) {
            const long long x_off = on_device ? (long long)off[u] * D : -1;
            printf("prob %d %d %d %d %d %lld\n", u, res[u].status, res[u].id, res[u].n_pos, res[u].n_neg, x_off);
            if (res[u].status == OWW_FIT_OK) { run.push_back(u); Ns.push_back((int)(off[u + 1] - off[u])); }
        }
        const std::vector<owf::Slab> slabs = owf::slab_plan(Ns, D, budget, on_device != 0);
        for (size_t s = 0; s < slabs.size(); ++s) {
            const owf::Slab& sl = slabs[s];
            printf("slab %d %d %lld %lld %lld\n", sl.first, sl.last, sl.rows, sl.k_floats, sl.tiles);
            const std::vector<owf::Tile> tiles = owf::tile_map(Ns, sl.first, sl.last);
            printf("tiles %zu %zu\n", s, tiles.size());
            for (size_t t = 0; t < tiles.size() && t < 64; ++t) printf("tile %zu %d %d %d\n", s, tiles[t].p, tiles[t].tr, tiles[t].tc);
        }
        free(labels);
    }
    return 0;
}
