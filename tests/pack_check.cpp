// pack_check -- runs the host-side weight packer (openwakeword_amd/csrc/owwhip_pack.h) on blobs from a directory and prints one line of
// fingerprints per case.  Stand-alone: no HIP, no GPU, not loaded into Python; tests/test_pack_host_cpu.py builds it with the host
// compiler under AddressSanitizer + UBSan and compares the lines with tests/golden/pack_fingerprints.json.
//
//   pack_check DIR        reads DIR/cases.txt, one case per line:
//     parse  NAME KIND FILE                 KIND = mel | emb | head | vad: the blob parser; `untouched` = a refused blob left the output alone
//     ladder NAME ABSMAX_FILE EMB_FILE      hx_ladder: the 46 scale exponents
//     bank   NAME HEAD_FILE PROBE_FILE|-    the packing sequence of oww_bank_add (first layer on its own, b3 inside the pad block)
//     image  NAME key=value ...             build_nets + the image phases of oww_commit; keys: family (valu | mfma | rr | hx), mel, emb,
//                                           vad (file or -), heads (comma list or -), probe (file or -), ladder (0 | 1), nowide (0 | 1), ring
#include "owwhip_pack.h"

#include <cstdint>
#include <fstream>
#include <iostream>
#include <map>
#include <sstream>

using namespace owp;

static std::string g_dir;

static std::vector<char> read_file(const std::string& name) {
    std::ifstream f(g_dir + "/" + name, std::ios::binary);
    if (!f) { fprintf(stderr, "pack_check: cannot read %s\n", name.c_str()); exit(2); }
    return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
static std::vector<float> read_floats(const std::string& name) {
    const std::vector<char> b = read_file(name);
    std::vector<float> v(b.size() / 4);
    if (!v.empty()) memcpy(v.data(), b.data(), v.size() * 4);
    return v;
}
static uint64_t fnv(const std::vector<float>& v) { return fp_mix(14695981039346656037ull, v.data(), v.size() * sizeof(float)); }
static std::string msg() { std::string m = g_err; for (char& c : m) if (c == ' ') c = '_'; return m; }

static void print_image(const std::vector<float>& v) { printf(" fnv=%016llx len=%zu", (unsigned long long)fnv(v), v.size()); }
static void print_pack(const HxNetPack& p) { printf(" [e1=%d e2=%d e3=%d eh=%d w2=%zu w3=%zu pad=%zu]", p.e1, p.e2, p.e3, p.eh, p.w2, p.w3, p.pad); }

// a blob parser on a pre-filled output: accepted -> fingerprint of what it stored, refused -> code, message, and whether the output is intact
static void case_parse(const std::string& kind, const std::string& file) {
    const std::vector<char> blob = read_file(file);
    const std::vector<float> mark = {1.f, 2.f, 3.f};
    if (kind == "head") {
        HeadHost hh{};
        hh.kind = -7; hh.blob = mark;
        const int rc = parse_head_blob("oww_add_head", blob.data(), blob.size(), 120, hh);
        printf(" rc=%d", rc);
        if (rc) printf(" untouched=%d msg=%s", (int)(hh.kind == -7 && hh.blob == mark), msg().c_str());
        else { printf(" kind=%d T=%d hidden=%d n_out=%d has_ln=%d n_blocks=%d", hh.kind, hh.T, hh.hidden, hh.n_out, hh.has_ln, hh.n_blocks); print_image(hh.blob); }
        return;
    }
    std::vector<float> out = mark;
    const int rc = kind == "mel" ? parse_mel_blob(blob.data(), blob.size(), out) :
                   kind == "emb" ? parse_embedding_blob(blob.data(), blob.size(), out) : parse_vad_blob(blob.data(), blob.size(), out);
    printf(" rc=%d", rc);
    if (rc) printf(" untouched=%d msg=%s", (int)(out == mark), msg().c_str());
    else print_image(out);
}

static void case_ladder(const std::string& absmax_file, const std::string& emb_file) {
    const std::vector<float> absmax = read_floats(absmax_file), emb = read_floats(emb_file);
    HxLadder o;
    hx_ladder(absmax.data(), emb, o);
    printf(" e=");
    for (int l = 0; l < 20; ++l) printf("%d,", o.hx_e[l]);
    printf(" ein=");
    for (int l = 0; l < 20; ++l) printf("%d,", o.hx_ein[l]);
    printf(" xexp=");
    for (int s = 0; s < 5; ++s) printf("%d,", o.hx_xexp[s]);
    printf(" efeat=%d", o.hx_efeat);
}

static void case_bank(const std::string& head_file, const std::string& probe_file) {
    const std::vector<char> blob = read_file(head_file);
    const std::vector<float> probe = probe_file == "-" ? std::vector<float>() : read_floats(probe_file);
    HeadHost hh{};
    int rc = parse_head_blob("oww_bank_add", blob.data(), blob.size(), 16, hh);
    printf(" rc=%d", rc);
    if (rc) { printf(" msg=%s", msg().c_str()); return; }
    NetHost net{};
    parse_dense_net(hh.blob.data(), hh.T, hh.hidden, 1, hh.has_ln, 1, net);
    const size_t K = (size_t)hh.T * 96;
    const int ht = hh.hidden <= 64 ? 4 : 8, HP = 16 * ht;
    HxNetPack pack;
    if (!hx_net_scales(net, ht, pack, probe, 1)) { printf(" not_finite"); return; }
    HostBuf hb;
    std::vector<float> wcat(K * HP, 0.f), pk;
    std::vector<double> colmul(HP);
    place_w1(net, 0, HP, HP, pack.e1, wcat, colmul);
    pack_hx_w1(wcat.data(), (int)K, HP, colmul.data(), pk);
    const size_t o_w1 = hb.add(pk);
    pack_hx_net(net, ht, true, hb, pack);
    printf(" ht=%d w1=%zu w1_floats=%zu", ht, o_w1, pk.size());
    print_pack(pack);
    print_image(hb.data);
    std::vector<float> win;
    const int B = probe_windows(probe, 1, hh.T, win);
    printf(" windows=%d f64=%.12g", B, bank_eval_f64(net, win.data()));
}

static void case_image(const std::map<std::string, std::string>& kv) {
    auto get = [&](const char* k, const char* dflt) { auto it = kv.find(k); return it == kv.end() ? std::string(dflt) : it->second; };
    PackIn in;
    const std::string fam = get("family", "hx");
    in.mfma = fam != "valu"; in.rr = fam == "rr" || fam == "hx"; in.hx = fam == "hx";
    in.no_wide_heads = get("nowide", "0") == "1";
    in.feature_ring = atoi(get("ring", "0").c_str());
    int rc = 0;
    { const std::vector<char> b = read_file(get("mel", "mel.bin")); rc = parse_mel_blob(b.data(), b.size(), in.mel_blob); }
    if (!rc) { const std::vector<char> b = read_file(get("emb", "emb.bin")); rc = parse_embedding_blob(b.data(), b.size(), in.emb_blob); }
    if (!rc && get("vad", "-") != "-") { const std::vector<char> b = read_file(get("vad", "-")); rc = parse_vad_blob(b.data(), b.size(), in.vad_blob); }
    std::stringstream hs(get("heads", "-"));
    for (std::string f; !rc && std::getline(hs, f, ',');) {
        if (f == "-") break;
        const std::vector<char> b = read_file(f);
        HeadHost hh{};
        if (!(rc = parse_head_blob("oww_add_head", b.data(), b.size(), 120, hh))) in.heads.push_back(std::move(hh));
    }
    if (rc) { printf(" load_rc=%d msg=%s", rc, msg().c_str()); return; }
    if (get("probe", "-") != "-") { in.probe_emb = read_floats(get("probe", "-")); in.probe_nb = 1; }
    if (get("ladder", "0") == "1") {                 // a fixed non-trivial ladder, consistent inside the stages and across the hand-overs
        const int first[5] = {0, 3, 7, 11, 15};
        for (int l = 0; l < 20; ++l) { in.hx_e[l] = (3 * l) % 5 - 2; in.hx_ein[l] = l == 0 ? 0 : in.hx_e[l - 1]; }
        for (int st = 1; st < 5; ++st) in.hx_ein[first[st]] = st % 3 - 1;
        in.hx_ein[19] = 1;
        for (int st = 0; st < 5; ++st) { const int last = st == 0 ? 2 : first[st] + 3; in.hx_xexp[st] = in.hx_ein[last + 1] - in.hx_e[last]; }
        in.hx_efeat = 2;
    }
    int NL = 0, TR = 0, hmax = 0;
    HostBuf hb;
    WeightOff off;
    HeadGroups hg;
    float vgain = 0.f, vbd = 0.f;
    rc = build_nets(in, NL, TR, hmax);
    if (!rc) rc = pack_mel_tables(in, hb, off);
    if (!rc) rc = pack_cnn(in, hb, off);
    if (!rc) { pack_net_arrays(in, hb, off); rc = pack_head_groups(in, hg, hb, off); }
    if (!rc) rc = pack_vad(in, hb, off, vgain, vbd);
    printf(" rc=%d", rc);
    if (rc) { printf(" msg=%s", msg().c_str()); return; }
    print_image(hb.data);
    printf(" NL=%d TR=%d hmax=%d mel=%zu,%zu,%zu,%zu,%zu conv=", NL, TR, hmax, off.hann, off.start, off.taps, off.meloff, off.meldst);
    for (int l = 0; l < 20; ++l) printf("%zu/%zu/%zu,", off.conv[l], off.scale[l], off.shift[l]);
    printf(" out_col=");
    for (const HeadHost& hh : in.heads) printf("%d,", hh.out_col);
    printf(" nets=");
    for (size_t i = 0; i < off.net.size(); ++i) {
        const WeightOff::Net& o = off.net[i];
        const NetHost& n = in.nets[i];
        printf("(h%d r%d c%d H%d O%d ln%d T%d act%d nb%d: %zu,%zu,%zu,%zu,%zu,%zu,%zu,%zu,%zu,%zu,%zu,%zu,%zu)", n.head, n.role, n.out_col, n.hidden, n.n_out, n.has_ln, n.T,
               n.final_act, n.n_blocks, o.w1, o.b1, o.ln1g, o.ln1b, o.w2, o.b2, o.ln2g, o.ln2b, o.w3, o.b3, o.w2pk, o.blocks, o.rnn);
    }
    printf(" head_nets=");
    for (const auto& hn : in.head_nets) printf("%d-%d,", hn.first, hn.second);
    printf(" groups=");
    for (size_t gi = 0; gi < hg.groups.size(); ++gi) {
        const HeadGroup& g = hg.groups[gi];
        const WeightOff::Group& go = off.group[gi];
        printf("{T=%d NH=%d n=%d ht=%d nets=", g.T, g.NH, g.n_nets, g.ht);
        for (int ni : g.nets) printf("%d,", ni);
        printf(" w1pk=%zu b1cat=%zu w1hx=%zu", go.w1pk, go.b1cat, go.w1hx);
        for (const HxNetPack& p : go.net) print_pack(p);
        printf("}");
    }
    printf(" generic=");
    for (int ni : hg.generic_nets) printf("%d,", ni);
    printf(" rnn=");
    for (int ni : hg.rnn_nets) printf("%d,", ni);
    printf(" vad=%zu,%zu,%zu,%zu,%zu,%zu gain=%.9g bd=%.9g", off.vhann, off.vencw, off.vencb, off.vlw, off.vlb, off.vwd, (double)vgain, (double)vbd);
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: pack_check DIR\n"); return 2; }
    g_dir = argv[1];
    std::ifstream cases(g_dir + "/cases.txt");
    if (!cases) { fprintf(stderr, "pack_check: no cases.txt in %s\n", argv[1]); return 2; }
    for (std::string line; std::getline(cases, line);) {
        std::stringstream ss(line);
        std::string what, name, a, b;
        if (!(ss >> what >> name)) continue;
        printf("%s", name.c_str());
        g_err.clear();
        if (what == "parse") { ss >> a >> b; case_parse(a, b); }
        else if (what == "ladder") { ss >> a >> b; case_ladder(a, b); }
        else if (what == "bank") { ss >> a >> b; case_bank(a, b); }
        else if (what == "image") {
            std::map<std::string, std::string> kv;
            for (std::string t; ss >> t;) { const size_t eq = t.find('='); if (eq != std::string::npos) kv[t.substr(0, eq)] = t.substr(eq + 1); }
            case_image(kv);
        }
        else { fprintf(stderr, "pack_check: unknown case kind %s\n", what.c_str()); return 2; }
        printf("\n");
        fflush(stdout);
    }
    return 0;
}
