// auto_train_check.cpp -- the host layer of device-side validation, checkpoints and merge as a plain host program:
// openwakeword_amd/csrc/owwhip_autotrain_host.h alone, no HIP, built with -fsanitize=address,undefined by
// tests/test_auto_train_cpu.py, which holds the output to the Python restatement of sizes, plan and refusals.
//   auto_train_check FILE   one case per line of FILE:
//       name open P EP C U T D source n shared tables scores Cnew slots dst gu gslot gn
//     open: a session is open; P: windows handed to set_eval_pool; EP: windows of the session's eval pool (0 = none); C: reserved
//     slots (0 = none); tables: ok, hi (an index = EP at the last entry), lo (-2 at the first), lab (a label 2 at the last entry);
//     scores: 0 / 1; Cnew: the argument of oww_train_checkpoints; slots: ok (u % C, -1 at u = 0), hi (C at the last), lo (-2 at the
//     first); dst: oww_train_average's; gu gslot gn: oww_train_get_slot's problem, slot and room (0 = the record's size, else that).
// Per case: "case NAME seq RC epool RC eval RC ckpt RC snap RC avg RC get RC", then (eval accepted) "plan n_tiles table scores" and
// (checkpoints accepted) "slots FLOATS".
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "owwhip_autotrain_host.h"

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: auto_train_check FILE\n"); return 2; }
    std::ifstream in(argv[1]);
    std::string line;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        std::istringstream ls(line);
        std::string name, tables, slots;
        int open, C, U, T, D, source, n, shared, scores, Cnew, dst, gu, gslot;
        long long P, EP, gn;
        ls >> name >> open >> P >> EP >> C >> U >> T >> D >> source >> n >> shared >> tables >> scores >> Cnew >> slots >> dst >> gu >> gslot >> gn;
        if (!ls) { fprintf(stderr, "auto_train_check: bad line '%s'\n", line.c_str()); return 2; }
        const float dummy = 0.f;                                      // windows and parameters are never read by the host layer
        const owt::Layout L = owt::layout(T, D);
        const int r_seq = owa::check_new_sequence(open != 0);
        const int r_pool = owa::check_eval_pool(open != 0, &dummy, P, T);
        oww_train_counts cnt{};
        int r_eval = owa::check_eval_head(open != 0, EP, C, source, n, reinterpret_cast<const int32_t*>(&dummy), reinterpret_cast<const uint8_t*>(&dummy), &cnt);
        if (r_eval == 0) {
            const owa::EvalPlan pl = owa::eval_plan(U, n, shared, scores != 0);
            // exactly the entries of the call on the heap, so that a read past them is seen
            std::vector<int32_t> idx((size_t)pl.table);
            std::vector<uint8_t> y((size_t)pl.table);
            for (size_t i = 0; i < idx.size(); ++i) { idx[i] = i % 7 == 3 ? -1 : (int32_t)(i % (size_t)EP); y[i] = (uint8_t)(i & 1); }
            if (tables == "hi") idx.back() = (int32_t)EP;
            if (tables == "lo") idx[0] = -2;
            if (tables == "lab") y.back() = 2;
            r_eval = owa::check_eval(open != 0, EP, C, U, source, n, idx.data(), y.data(), shared, &cnt);
        }
        long long floats = -1;
        const int r_ckpt = owa::check_checkpoints(open != 0, Cnew, U, L.stride, &floats);
        std::vector<int32_t> slot((size_t)U);
        for (int u = 0; u < U; ++u) slot[(size_t)u] = u == 0 || C < 1 ? -1 : u % C;
        if (slots == "hi") slot.back() = C;
        if (slots == "lo") slot[0] = -2;
        const int r_snap = owa::check_snapshot(open != 0, C, U, slot.data());
        const std::vector<uint8_t> sel((size_t)U * (size_t)(C > 0 ? C : 1), 1);
        const int r_avg = owa::check_average(open != 0, C, sel.data(), dst);
        float room = 0.f;
        const int r_get = owa::check_get_slot(open != 0, C, U, gu, gslot, &room, gn ? gn : L.n, L.n);
        printf("case %s seq %d epool %d eval %d ckpt %d snap %d avg %d get %d\n", name.c_str(), r_seq, r_pool, r_eval, r_ckpt, r_snap, r_avg, r_get);
        if (r_eval == 0) {
            const owa::EvalPlan pl = owa::eval_plan(U, n, shared, scores != 0);
            printf("plan %d %lld %lld\n", pl.n_tiles, pl.table, pl.scores);
        }
        if (r_ckpt == 0) printf("slots %lld\n", floats);
    }
    return 0;
}
