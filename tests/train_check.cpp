// train_check.cpp -- the host layer of device-side head training as a plain host program: openwakeword_amd/csrc/owwhip_train_host.h
// alone, no HIP, built with -fsanitize=address,undefined by tests/test_head_train_cpu.py, which holds the output to the Python
// restatement of layout, plan and refusals.
//   train_check FILE   one case per line of FILE:  name committed open U T D TR P K n shared tables lr nw
//                      tables: ok, hi (an index = P at the last entry), lo (-2 at the first), lab (a label 2 at the last entry);
//                      lr / nw as text ("nan" and "inf" must get through), put at step K - 1 of otherwise 1e-3 / 1 schedules
// Per case: "case NAME begin RC pool RC steps RC", then (begin accepted) "layout F D w1 b1 g1 be1 w2 b2 g2 be2 w3 b3 n stride small"
// and (steps accepted) "plan n_tiles n_pad dz1 part tile_words w1_groups".
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "owwhip_train_host.h"

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: train_check FILE\n"); return 2; }
    std::ifstream in(argv[1]);
    std::string line;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        std::istringstream ls(line);
        std::string name, tables, lr_text, nw_text;
        int committed, open, U, T, D, TR, K, n, shared;
        long long P;
        ls >> name >> committed >> open >> U >> T >> D >> TR >> P >> K >> n >> shared >> tables >> lr_text >> nw_text;
        if (!ls) { fprintf(stderr, "train_check: bad line '%s'\n", line.c_str()); return 2; }
        const float dummy = 0.f;                                      // parameters and windows are never read by the host layer
        const int rb = owt::check_begin(committed != 0, open != 0, U, T, D, TR, &dummy);
        const int rp = rb == 0 ? owt::check_pool(true, &dummy, P, T) : -99;
        int rs = -99;
        if (rb == 0 && rp == 0) {
            const bool sized = K >= 1 && K <= owt::kMaxSteps && n >= 1 && n <= owt::kMaxBatch;
            const size_t total = sized ? (size_t)(shared ? 1 : U) * K * n : 1;
            // exactly the entries of the call on the heap, so that a read past them is seen
            std::vector<int32_t> idx(total);
            std::vector<uint8_t> y(total);
            for (size_t i = 0; i < total; ++i) { idx[i] = (int32_t)(i % (size_t)P); y[i] = (uint8_t)(i & 1); }
            if (tables == "hi") idx[total - 1] = (int32_t)P;
            if (tables == "lo") idx[0] = -2;
            if (tables == "lab") y[total - 1] = 2;
            std::vector<double> lr((size_t)(sized ? K : 1), 1e-3);
            std::vector<float> nw((size_t)(sized ? K : 1), 1.f);
            lr.back() = strtod(lr_text.c_str(), nullptr);
            nw.back() = strtof(nw_text.c_str(), nullptr);
            oww_train_record out{};
            rs = owt::check_steps(true, P, U, K, n, idx.data(), y.data(), shared, lr.data(), nw.data(), &out);
        }
        printf("case %s begin %d pool %d steps %d\n", name.c_str(), rb, rp, rs);
        if (rb) continue;
        const owt::Layout L = owt::layout(T, D);
        printf("layout %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld\n", L.F, L.D, L.w1, L.b1, L.g1, L.be1, L.w2, L.b2, L.g2,
               L.be2, L.w3, L.b3, L.n, L.stride, L.small);
        if (rs) continue;
        const owt::Plan p = owt::plan(U, T, D, n);
        printf("plan %d %d %lld %lld %lld %d\n", p.n_tiles, p.n_pad, p.dz1, p.part, p.tile_words, p.w1_groups);
    }
    return 0;
}
