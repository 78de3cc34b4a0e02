// owwhip.hip -- host side of libowwhip.so: context, weight packing, kernel launches, C ABI.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -shared -fPIC owwhip.hip -I../../include -o libowwhip.so
// Interface contract and the reference call sites each entry replaces: include/owwhip.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <exception>
#include <mutex>
#include <new>
#include <unordered_map>
#include <dlfcn.h>
#include <string>
#include <vector>

#include "owwhip.h"
#include "owwhip_pack.h"
#include "owwhip_ingest.h"
#include "owwhip_mem.h"
#include "owwhip_masked_host.h"
#include "owwhip_bank_host.h"
#include "owwhip_verifier_host.h"
#include "owwhip_state_host.h"
#include "owwhip_postproc.h"
#include "owwhip_kernels.h"
#include "owwhip_rr.h"
#include "owwhip_hx.h"
#include "owwhip_vad.h"
#include "owwhip_fused.h"
#include "owwhip_state.h"
#include "owwhip_events.h"
#include "owwhip_audio.h"
#include "owwhip_dense.h"
#include "owwhip_dense_hits_host.h"
#include "owwhip_fit.h"
#include "owwhip_train.h"
#include "owwhip_autotrain.h"

using namespace owk;
using namespace owp;
using owm::DevBuf;
using owm::PinnedBuf;

namespace {

// Nothing throws across the C ABI: every extern "C" body that can allocate (std::vector / std::string packing buffers, new) runs
// between these two, which turn a C++ exception into an error code + message like any other failure.
#define OWW_GUARD_BEGIN try {
#define OWW_GUARD_END                                                                                              \
    } catch (const std::bad_alloc&) { return fail(OWW_ENOMEM, "%s: out of host memory", __func__);                 \
    } catch (const std::exception& e__) { return fail(OWW_ESTATE, "%s: unexpected C++ exception: %s", __func__, e__.what()); \
    } catch (...) { return fail(OWW_ESTATE, "%s: unexpected C++ exception", __func__); }

#define HIPCHK(expr)                                                                         \
    do {                                                                                     \
        hipError_t e__ = (expr);                                                             \
        if (e__ != hipSuccess) return fail(OWW_EHIP, "%s failed: %s", #expr, hipGetErrorString(e__)); \
    } while (0)

// ---- device allocations.  OWW_GUARD_ALLOC=1|2 is a debugging aid: every device buffer of the library then lives in its own
// virtual range (hipMemAddressReserve / hipMemMap) with an UNMAPPED granule on both sides and the buffer pushed against the upper (1)
// or the lower (2) end of its mapping, so that a kernel that reads or writes outside a buffer faults on the spot instead of touching
// whatever hipMalloc happened to place next to it; each allocation prints its address range and the source line that made it.
struct GuardRange { char* base; size_t reserve, mapped; hipMemGenericAllocationHandle_t hnd; };
std::mutex g_guard_mu;
std::unordered_map<void*, GuardRange> g_guard;
int guard_mode() {
    static const int mode = [] { const char* e = getenv("OWW_GUARD_ALLOC"); return e ? atoi(e) : 0; }();
    return mode;
}
hipError_t guard_alloc(void** p, size_t n, int line) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    hipMemAllocationProp prop = {};
    prop.type = hipMemAllocationTypePinned;
    prop.location.type = hipMemLocationTypeDevice;
    prop.location.id = dev;
    size_t gran = 0;
    if ((e = hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityMinimum)) != hipSuccess) return e;
    GuardRange g{};
    g.mapped = (std::max<size_t>(n, 1) + gran - 1) / gran * gran;
    g.reserve = g.mapped + 2 * gran;
    void* base = nullptr;
    if ((e = hipMemAddressReserve(&base, g.reserve, gran, nullptr, 0)) != hipSuccess) return e;
    g.base = static_cast<char*>(base);
    if ((e = hipMemCreate(&g.hnd, g.mapped, &prop, 0)) != hipSuccess) { (void)hipMemAddressFree(base, g.reserve); return e; }
    hipMemAccessDesc acc = {};
    acc.location = prop.location;
    acc.flags = hipMemAccessFlagsProtReadWrite;
    if ((e = hipMemMap(g.base + gran, g.mapped, 0, g.hnd, 0)) != hipSuccess ||
        (e = hipMemSetAccess(g.base + gran, g.mapped, &acc, 1)) != hipSuccess) {
        (void)hipMemRelease(g.hnd); (void)hipMemAddressFree(base, g.reserve); return e;
    }
    char* user = guard_mode() == 2 ? g.base + gran : g.base + gran + g.mapped - (n + 15) / 16 * 16;
    fprintf(stderr, "[owwhip guard] line %d: %zu bytes at [%p, %p), mapped [%p, %p)\n", line, n, (void*)user, (void*)(user + n),
            (void*)(g.base + gran), (void*)(g.base + gran + g.mapped));
    std::lock_guard<std::mutex> lk(g_guard_mu);
    g_guard[user] = g;
    *p = user;
    return hipSuccess;
}
hipError_t dev_alloc(void** p, size_t n, int line) {
    if (!guard_mode()) return hipMalloc(p, n);
    return guard_alloc(p, n, line);
}
hipError_t dev_free(void* p) {
    if (!guard_mode() || !p) return hipFree(p);
    GuardRange g;
    {
        std::lock_guard<std::mutex> lk(g_guard_mu);
        auto it = g_guard.find(p);
        if (it == g_guard.end()) return hipFree(p);
        g = it->second;
        g_guard.erase(it);
    }
    (void)hipDeviceSynchronize();
    const size_t gran = (g.reserve - g.mapped) / 2;
    (void)hipMemUnmap(g.base + gran, g.mapped);
    (void)hipMemRelease(g.hnd);
    return hipMemAddressFree(g.base, g.reserve);
}
}  // namespace

// ---- owwhip_mem.h's seam: what DevBuf / PinnedBuf / Event / Stream release goes through here and nowhere else
namespace owm {
int dev_alloc_raw(void** p, size_t bytes, int line) { return dev_alloc(p, bytes, line); }
int dev_free_raw(void* p) { return dev_free(p); }
int pinned_alloc_raw(void** p, size_t bytes, unsigned flags) { return hipHostMalloc(p, bytes, flags); }
int pinned_free_raw(void* p) { return hipHostFree(p); }
int event_create_raw(hipEvent_t* e, unsigned flags) { return hipEventCreateWithFlags(e, flags); }
int event_destroy_raw(hipEvent_t e) { return hipEventDestroy(e); }
int stream_create_raw(hipStream_t* s, unsigned flags) { return hipStreamCreateWithFlags(s, flags); }
int stream_destroy_raw(hipStream_t s) { return hipStreamDestroy(s); }
}  // namespace owm

namespace {
inline hipError_t herr(int e) { return static_cast<hipError_t>(e); }      // (the seam's codes are the runtime's)

// Copies between host memory and a hipMemMap'ed range: the runtime's path for PAGEABLE host memory drops bytes at some sizes /
// alignments (tools/experiments/vmm_copy_probe.hip: 5,000,000 bytes from a range that ends at its mapping's end), its pinned path does
// not -- under OWW_GUARD_ALLOC host <-> device copies therefore go through a page-locked bounce buffer, synchronously.
hipError_t guard_copy(void* dst, const void* src, size_t n, hipMemcpyKind kind, hipStream_t st) {
    PinnedBuf<char> pin;
    hipError_t e = herr(pin.alloc(n, hipHostMallocDefault));
    if (e != hipSuccess) return e;
    if (kind == hipMemcpyHostToDevice) {
        memcpy(pin, src, n);
        e = hipMemcpyAsync(dst, pin, n, kind, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
    } else {
        e = hipMemcpyAsync(pin, src, n, kind, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e == hipSuccess) memcpy(dst, pin, n);
    }
    return e;
}
inline hipError_t copy_async(void* dst, const void* src, size_t n, hipMemcpyKind kind, hipStream_t st) {
    if (guard_mode() && n && (kind == hipMemcpyHostToDevice || kind == hipMemcpyDeviceToHost)) return guard_copy(dst, src, n, kind, st);
    return hipMemcpyAsync(dst, src, n, kind, st);
}
inline hipError_t copy_sync(void* dst, const void* src, size_t n, hipMemcpyKind kind) {
    if (guard_mode() && n && (kind == hipMemcpyHostToDevice || kind == hipMemcpyDeviceToHost)) return guard_copy(dst, src, n, kind, nullptr);
    const hipError_t e = hipMemcpy(dst, src, n, kind);
    // (set-up time only: the consumers run on non-blocking streams, which nothing orders behind the legacy stream)
    return e != hipSuccess || kind != hipMemcpyHostToDevice ? e : hipStreamSynchronize(nullptr);
}

constexpr int kSmallLaunchWgs = 2 * 256;      // stage / heads launches of at most two workgroups per CU (MI355X: 256 CUs) use the deep weight rings
// stage B with its weights resident in LDS (owwhip_hx.h: hstage_kernel NS = 1): one persistent workgroup per CU, from this many groups
// (= streams) on: the smallest size of the sweep 4,096 .. 131,072 in profiles/r07_resident_b_ab.txt at which stage B AND the step
// read lower than with the ring kernels in every repeat (8,192: B 0.089 -> 0.082 ms, step 0.485 -> 0.481; at 4,096 stage B reads
// 2-3 us lower but the step does not resolve from its own repeats)
constexpr int kResidentBMinGroups = 8192;
constexpr int kResidentBWgs = 256;

struct FastGroup : HeadGroup {           // + where bind_weights put the group's pieces on the device
    DevBuf<NetDesc> d_nets;
    const float* d_w1pk = nullptr;    // (this and the next two: views into d_w)
    const float* d_b1cat = nullptr;
    const float* d_w1hx = nullptr;    // fp16-split k-step-major layer-1 weights (heads_hx_kernel)
    std::vector<owh::HeadHxNet> hx_net;   // per net: what the kernel reads behind the first layer (make_hx_net; built once at commit)
};

// The kernel's view of a packed net whose image starts at img (device).  b3: the narrow form's output bias where the pad block has none.
owh::HeadHxNet make_hx_net(const NetHost& n, int ht, const HxNetPack& p, const float* img, const float* b3, int hx_efeat) {
    const int HP = 16 * ht;
    const float* pd = img + p.pad;
    owh::HeadHxNet o{};
    o.w2hx = img + p.w2; o.b1 = pd; o.ln1g = pd + HP; o.ln1b = pd + 2 * HP; o.b2 = pd + 3 * HP; o.ln2g = pd + 4 * HP; o.ln2b = pd + 5 * HP;
    if (ht == 4) { o.w3 = pd + 6 * HP; o.b3 = b3 ? b3 : pd + 7 * HP; }
    else { o.b3 = pd + 6 * HP; o.w3hx = img + p.w3; o.u3 = std::ldexp(1.0f, -p.e3); }
    o.has_ln = n.has_ln; o.role = n.role; o.head = n.head; o.out_col = n.out_col;
    o.hidden = n.hidden; o.inv_hidden = 1.0f / (float)n.hidden;
    o.u1 = std::ldexp(1.0f, -(hx_efeat + p.e1) + (n.has_ln ? 0 : p.eh)); o.u2 = std::ldexp(1.0f, -(p.e2 + p.eh));
    o.n_out = n.n_out; o.final_act = n.final_act;
    return o;
}

struct EventRec { owm::Event a, b; int cls = 0; };

}  // namespace

struct oww_ctx : PackIn {                 // (PackIn: the weights as loaded, the family flags mfma / rr / hx, the f16-split scales)
    // Teardown (~oww_ctx): the body drains the three streams and releases communicator and graph, then the members release themselves
    // in reverse order of declaration -- the streams, declared first, go last.  stream: the caller's (cfg.stream, borrowed) or our own.
    owm::Stream stream, up_stream, down_stream;   // (up / down: the host-fed pipeline's uploads and score downloads)
    oww_config cfg{};
    int S = 0, Spad = 0, kmax = 1, TR = 16, NL = 0;
    bool committed = false;
    const int* state_len = kStateLenRr;
    ~oww_ctx();
    // device weights; the const pointers below are views into d_w
    DevBuf<float> d_w;
    const float *d_hann = nullptr, *d_taps = nullptr;
    const int* d_mstart = nullptr;
    const int* d_meloff = nullptr; const unsigned* d_meldst = nullptr;   // fused front end: compact tap table (oww_commit)
    const float* d_conv[20] = {};     // layer 0: natural [9][24]; 1..19: packed (mfma) or natural (valu)
    const float* d_scale[20] = {};
    const float* d_shift[20] = {};
    DevBuf<NetDesc> d_allnets;
    std::vector<FastGroup> groups;
    std::vector<int> generic_nets;    // indices into nets (with verifier right after its primary)
    std::vector<int> rnn_nets;        // recurrent heads (train.py:85-98): owk::heads_rnn_kernel, one launch per head
    int generic_hmax = 0;
    int generic_spw = 0;              // OWW_GENERIC_SPW: 4 / 16 pins the generic heads kernel's shape, 0 = by launch size
    // state
    DevBuf<float> d_state[N_STATE], d_tmpl[N_STATE];
    DevBuf<float> d_xA, d_xB, d_xC, d_xD;
    DevBuf<float> d_mel, d_feat, d_emb, d_raw, d_scores, d_ring;
    // host-fed pipeline (oww_submit / oww_collect): two steps in flight, uploads and score downloads on their own streams
    struct IngestSlot {
        DevBuf<int16_t> d_pcm; DevBuf<float> d_scores; PinnedBuf<float> h_scores;
        DevBuf<char> d_mix;          // oww_submit_ingest_mixed: [S][row_bytes] in the streams' own formats, allocated at first use
        PinnedBuf<uint8_t> h_on;     // page-locked staging of a masked submit's participation mask
        owm::Event up, done, down;
        bool busy = false;
    } slot[2];
    // detection events (oww_events_*; owwhip_events.h): one buffer set for the synchronous calls and one per ingest slot, the latter
    // with page-locked mirrors of counts and records that ride down behind the slot's scores
    struct EventBuf {
        DevBuf<oww_event> d_rec; DevBuf<int> d_count; DevBuf<float> d_snap;     // [cap + 1], {n_stored, n_total}, [cap + 1][rows][96]
        DevBuf<int16_t> d_asnap;                                                // [cap + 1][event_chunks][1280] (oww_audio_configure)
        PinnedBuf<oww_event> h_rec; PinnedBuf<int> h_count;                     // ingest slots only
    };
    int evt_cap = 0, evt_rows = 0;               // 0 = no events (oww_events_configure)
    DevBuf<float> d_evt_thr; float evt_bank_thr = 0.5f;
    DevBuf<int> d_evblock; int evt_blocks = 0;
    EventBuf evt_sync, evt_slot[2];
    const EventBuf* evt_cur = nullptr;           // what oww_get_events refers to: the last synchronous call or the last collected step
    // per-stream audio rings (oww_audio_configure; owwhip_audio.h, owwhip_audio_host.h): nothing without it
    int aud_ring = 0, aud_evt = 0;               // ring_chunks (0 = no audio), event_chunks
    DevBuf<int16_t> d_aring;                     // [S][aud_ring][1280]
    DevBuf<uint32_t> d_acount;                   // [S] chunks since the stream's reset
    DevBuf<int16_t> d_aout; DevBuf<int> d_aids; DevBuf<uint32_t> d_acnt;   // oww_get_audio: staging of a host read, the list, the counters

    uint64_t n_submit = 0, n_collect = 0;
    DevBuf<float> d_featinit, d_dbg;
    DevBuf<long long> d_prof;        // [4 stages][16 waves][16 marks], allocated when OWW_PROF_BLOCK is set
    int prof_block = -1;
    DevBuf<uint32_t> d_nfeat, d_npred, d_nvad;
    DevBuf<float> d_vadring, d_vadin; float vad_threshold = 0.f;   // VAD gate (oww_push_vad)
    // voice-activity stand-in network on the device (oww_load_vad; owwhip_vad.h)
    bool vad = false;
    const float *d_vad_hann = nullptr, *d_vad_encw = nullptr, *d_vad_encb = nullptr, *d_vad_lstmw = nullptr, *d_vad_lstmb = nullptr, *d_vad_wd = nullptr;
    float vad_bd = 0.f, vad_gain = 50.f;
    DevBuf<float> d_vadx, d_vadhc, d_vadlast;
    DevBuf<int16_t> d_tail, d_pcm;
    DevBuf<int16_t> d_long;          // oww_step with n_chunks > max_chunks: the whole call's PCM when it arrives from the host
    DevBuf<float> d_callmax;         // ... and the call's per-stream mel maximum (launch_step_long)
    PinnedBuf<int> h_range;          // sticky f16-range flag: one page-locked, device-mapped word the f16-split kernels raise
    int* d_range = nullptr;          // the same word as the kernels address it (a view: the device alias of h_range)
    DevBuf<char> d_rs;               // oww_resample scratch: [taps | in | out] as needed, in bytes
    std::vector<float> rs_taps;                    // the padded filter bank of the last oww_resample call (upload source)
    // stateful stream ingest: nothing before the first configure.  The single form (oww_ingest_configure; owk::ingest_kernel) is a table
    // of one row served by its own kernel, the class form (oww_ingest_configure_classes; owk::ingest_mixed_kernel) sets `mixed` and
    // has the table and the class ids on the device as well.
    struct Ingest {
        bool ready = false, mixed = false;
        owi::Table tab;                            // host copy of the rows and padded banks (upload source, fingerprint, checks)
        DevBuf<float> d_taps;                      // every bank (none: single form, decode only)
        DevBuf<int16_t> d_hist;                    // [S][tab.Hpad_max]: each stream's last n_taps - 1 decoded samples, oldest first, zero padded
        DevBuf<int16_t> d_out;                     // 16 kHz staging [S][n_out] (oww_ingest_dev), grown on demand; survives reconfiguration
        DevBuf<char> d_in;                         // a host message on its way in, in bytes
        DevBuf<uint8_t> d_on;                      // [S] a host mask on its way in
        DevBuf<IngestClass> d_table;               // class form: the rows
        DevBuf<uint32_t> d_cls;                    // class form: [S] each stream's class, a word per stream, so that the state records carry it
        DevBuf<int> d_newcls;                      // the class list of oww_ingest_assign on its way in
    } ing;
    DevBuf<uint8_t> d_on;            // oww_step_masked: [Spad] participation mask of the step being launched (pad streams 0)
    // masked step with few participants: the device copy of the group lists (StepArgs::gl) and its two page-locked staging buffers,
    // used in turn (build_active_lists)
    DevBuf<int> d_lists; PinnedBuf<int> h_lists[2]; owm::Event lists_ev[2]; unsigned lists_turn = 0;
    int k_last = 1;                  // n_chunks of the last step (row stride of d_mel)
    float hx_absmax[20] = {};        // largest |activation| of each layer in the calibration run (exact-fp32 kernels)
    std::vector<int16_t> cal_user;   // oww_set_calibration: caller's calibration audio as [n_seg][CAL_T * 1280] segments
    int small_wgs = kSmallLaunchWgs, small_wgs_heads = kSmallLaunchWgs;   // A/B aids: OWW_SMALL_WGS / OWW_SMALL_WGS_HEADS (0 = never the deep rings)
    int resident_b = -1, resident_b_wgs = kResidentBWgs;                  // OWW_RESIDENT_B=0|1|auto (-1 = auto: by size), OWW_RESIDENT_B_WGS = grid cap
    float hx_selftest_err = 0.f, hx_selftest_ref = 0.f, hx_selftest_score_err = 0.f;   // commit-time f16-split vs exact-fp32 comparison
    bool fuse = false;               // f16-split family: mel front end fused into stage A for one-chunk streaming steps (owwhip_fused.h)
    // custom verifiers on the device (oww_set_verifier)
    DevBuf<float> d_verw, d_verb, d_verthr; DevBuf<int> d_verT;
    int ver_stride = 0, n_verifiers = 0;
    std::vector<int> ver_T;
    bool post_in_heads = false;          // one group of sigmoid heads covers every label: post-processing + counter advance ride in the heads launch
    DevBuf<float> d_save;                // streaming state parked by oww_embed / oww_embed_clips
    DevBuf<int> d_ids;                   // the stream ids of oww_reset / oww_reset_vad (upload_ids)
    DevBuf<int> d_patience;
    DevBuf<float> d_threshold;
    int debounce_frames = 0;
    // RCCL communicator of oww_comm_init (multi-GPU delivery of results without Python)
    void* comm = nullptr; int comm_rank = 0, comm_world = 1;
    // timing
    bool timing = false;
    std::vector<EventRec> ev;
    size_t ev_used = 0;
    double t_ms[OWW_N_KERNEL_CLASSES] = {};
    int64_t t_n[OWW_N_KERNEL_CLASSES] = {};
    // graph
    bool want_graph = false;
    hipGraph_t graph = nullptr;
    hipGraphExec_t graph_exec = nullptr;
    // head bank (oww_bank_*): routed f16-split heads, each stream subscribed to up to bank_K of them (owh::heads_bank_kernel)
    struct BankHead {
        bool live = false;
        int T = 0, hidden = 0, has_ln = 0, ht = 4, patience = 0;
        float threshold = NAN;
        DevBuf<float> d_img;                     // w1hx | the pieces of pack_hx_net: the packing of a fixed net of the same width
        size_t w1_bytes = 0;                     // first-layer weight bytes one tile streams
        owh::BankHeadDev dev{};
    };
    int bank_K = 0, bank_cap = 0;                // 0 = no bank (oww_bank_configure)
    std::vector<BankHead> bank;
    std::vector<int> bank_sub;                   // host copy of d_bank_sub: [S][K] bank head per slot, -1 = empty
    DevBuf<int> d_bank_sub, d_bank_idx;
    DevBuf<float> d_bank_raw, d_bank_scores, d_bank_ring;
    DevBuf<uint32_t> d_bank_npred;
    DevBuf<owh::BankHeadDev> d_bank_heads; DevBuf<int> d_bank_pat; DevBuf<float> d_bank_thr;
    DevBuf<owh::BankTile> d_bank_tiles; DevBuf<int> d_bank_entries;
    owb::Route bank_rt;                          // the routing table as uploaded (bank_route; owwhip_bank_host.h)
    // per-stream custom verifiers (oww_verifier_*): a pool of folded verifiers, one (verifier, threshold) per (stream, fixed column) and
    // per (stream, bank slot), and the device list of the pairs to verify that stream_verifier_kernel walks
    int vpool_cap = 0;                           // 0 = not configured (oww_verifier_configure)
    int vpool_stride = 0;                        // floats per pool entry: feature ring x 96
    std::vector<int> vpool_T;                    // [cap] feature rows of each pool verifier; 0 = free
    DevBuf<float> d_vpool_w, d_vpool_b;
    std::vector<int> vasg_fix, vasg_bank;        // [S][NL], [S][K]: pool id, OWW_VERIFIER_DEFAULT or OWW_VERIFIER_NONE
    std::vector<float> vthr_fix, vthr_bank;      // thresholds of the pool assignments
    long long vasg_n = 0;                        // pairs whose assignment is not the default: > 0 switches to stream_verifier_kernel
    std::vector<float> ver_thr;                  // host copy of d_verthr (the handle-wide verifiers' thresholds)
    DevBuf<SvEntry> d_svlist; int sv_n = 0;      // [S * (NL + K)] capacity; sv_n entries in use
    DevBuf<unsigned long long> d_sv_eval;        // evaluations of the last step
    // oww_verifier_fit's scratch (owwhip_fit.h), grown by the first call that needs it: nothing before that
    struct FitScratch {
        DevBuf<float> x, K, a, b;
        DevBuf<uint16_t> zh, zl;                 // (f16 bits)
        DevBuf<double> mu, sd;
        DevBuf<unsigned char> y;
        DevBuf<int> flag;
        DevBuf<owf::Record> rec;
        DevBuf<owf::Problem> prob;
        DevBuf<owf::Tile> tiles;
    } fit;
    // the head-training session (oww_train_*; owwhip_train.h): allocated by oww_train_begin, released by oww_train_end
    struct TrainSession {
        bool open = false;
        int U = 0, T = 0, D = 0;
        int64_t P = 0;
        owt::Layout L{};
        DevBuf<float> par, am, av, pool, dz1, part, tloss, nw;
        DevBuf<double> lr;
        DevBuf<owt::Counters> cnt;
        DevBuf<int> idx, tcount;
        DevBuf<unsigned char> y;
        DevBuf<owt::StepRecord> rec;
        // validation, checkpoints and merge (oww_train_eval ..; owwhip_autotrain.h): nothing of this before the entries are called
        int64_t EP = 0;
        int C = 0;
        DevBuf<float> epool, ckpt, escores;
        DevBuf<int> eidx, ecounts, slot;
        DevBuf<unsigned char> ey, sel;
    } train;
    // stream state records (oww_state_*, oww_move_streams; owwhip_state.h): built by the first of those calls, nothing before it
    bool st_ready = false;
    std::vector<ows::FlatSection> st_flat;       // host copy of d_st_flat
    std::vector<ows::GroupSection> st_group;     // (live: a view)
    bool st_levels[4] = {};                      // which of ows::kStateLevels a group section uses
    DevBuf<ows::FlatSection> d_st_flat;
    uint32_t st_record_words = 0, st_flat_quads = 0;
    uint64_t st_fp = 0;                          // fingerprint of family, layouts, ring sizes, scales and weights
    DevBuf<int> d_st_items;                      // [ids | group items per level] of the call being served
    DevBuf<uint32_t> d_st_stage;                 // records in flight between a host buffer / the two halves of a move
};

namespace {

// What the launches of one step (or embedding / probe run) need beyond the handle.  The entry points build it and pass it down by
// const reference; no launch helper reads a mode that a caller left behind in the handle.
struct StepArgs {
    const uint8_t* on = nullptr;          // masked step: participation mask (d_on, pad streams 0); nullptr = every stream
    // masked step with few participants (build_active_lists): the launches of stages B..E, the heads and the VAD LSTM cover only the
    // listed groups.  gl[0] = stream ids (stage B's groups and the heads' positions), [1] C, [2] D, [3] E, [4] VAD LSTM; gn = lengths
    bool lists = false;
    const int* gl[5] = {};
    int gn[5] = {};
    const int16_t* fused_pcm = nullptr;   // fused one-chunk step: stage A computes its mel rows from this PCM (owwhip_fused.h)
    bool post_in_heads = false;           // post-processing + counter advance ride in the heads launch (one-chunk steps only)
    const float* mel = nullptr;           // the CNN reads its mel rows from here (oww_embed_clips); nullptr = d_mel
    bool dbg = false;                     // per-layer dump into d_dbg (debug_layers handles)
};

// a step over every stream, mel rows from d_mel, per-layer dumps where the handle keeps them
StepArgs step_args(const oww_ctx* h) { StepArgs a; a.dbg = h->d_dbg != nullptr; return a; }

int flush_events(oww_ctx* h) {
    if (!h->ev_used) return 0;
    HIPCHK(hipStreamSynchronize(h->stream));
    for (size_t i = 0; i < h->ev_used; ++i) {
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, h->ev[i].a, h->ev[i].b));
        h->t_ms[h->ev[i].cls] += ms;
        h->t_n[h->ev[i].cls] += 1;
    }
    h->ev_used = 0;
    return 0;
}

struct Timed {          // RAII: records a start event now and a stop event at scope exit
    oww_ctx* h;
    EventRec* r = nullptr;
    Timed(oww_ctx* h_, int cls) : h(h_) {
        if (!h->timing) return;
        if (h->ev_used == h->ev.size()) {
            if (h->ev.size() >= 8192) { flush_events(h); }
            else {
                EventRec e;
                if (e.a.create(hipEventDefault) || e.b.create(hipEventDefault)) return;
                h->ev.push_back(std::move(e));
            }
        }
        r = &h->ev[h->ev_used++];
        r->cls = cls;
        (void)hipEventRecord(r->a, h->stream);
    }
    ~Timed() { if (r) (void)hipEventRecord(r->b, h->stream); }
};

template <class K>
int set_lds(K kernel, int bytes) {
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    return 0;
}

// ---- CNN over the first n_active streams, mel rows at d_mel + s*mel_stride + mel_off ----------------
template <bool MFMA>
int run_cnn_t(oww_ctx* h, const StepArgs& a, int n_active, int mel_stride, int mel_off) {
    hipStream_t st = h->stream;
    const bool dbg = a.dbg;
    int off = 0;
    int dbg_off[20];
    for (int l = 0; l < 20; ++l) { dbg_off[l] = off; off += kLayerOut[l][0] * kLayerOut[l][1] * kLayerOut[l][2]; }
    {
        StageAParams p{};
        p.mel = a.mel ? a.mel : h->d_mel; p.mel_stride = mel_stride; p.mel_off = mel_off;
        p.hist_mel = h->d_state[0]; p.hist2 = h->d_state[1];
        p.w0 = h->d_conv[0]; p.w1 = h->d_conv[1]; p.w2 = h->d_conv[2];
        for (int i = 0; i < 3; ++i) { p.scale[i] = h->d_scale[i]; p.shift[i] = h->d_shift[i]; p.dbg_off[i] = dbg_off[i]; }
        p.xout = h->d_xA; p.dbg = dbg ? h->d_dbg : nullptr; p.dbg_stride = DBG_FLOATS;
        Timed t(h, 1);
        hipLaunchKernelGGL(stageA_kernel<MFMA>, dim3(n_active), dim3(CfgA::NT), CfgA::LDS_BYTES, st, p);
    }
    auto fill = [&](StageParams& p, const float* xin, float* xout, int first_layer, int sb, int sd) {
        p.xin = xin; p.xout = xout; p.hist_b = h->d_state[sb]; p.hist_d = h->d_state[sd];
        for (int i = 0; i < 4; ++i) {
            p.w[i] = h->d_conv[first_layer + i]; p.scale[i] = h->d_scale[first_layer + i];
            p.shift[i] = h->d_shift[first_layer + i]; p.dbg_off[i] = dbg_off[first_layer + i];
        }
        p.dbg = dbg ? h->d_dbg : nullptr; p.dbg_stride = DBG_FLOATS;
        p.prof = h->d_prof ? h->d_prof + (first_layer / 4) * 256 : nullptr;      // first_layer 3,7,11,15 -> slot 0..3
        p.prof_block = h->prof_block;
    };
    {
        StageParams p{}; fill(p, h->d_xA, h->d_xB, 3, 2, 3);
        Timed t(h, 2);
        hipLaunchKernelGGL((stage_kernel<CfgB, MFMA, false>), dim3((n_active + CfgB::B - 1) / CfgB::B), dim3(CfgB::NT), CfgB::LDS_BYTES, st, p);
    }
    {
        StageParams p{}; fill(p, h->d_xB, h->d_xC, 7, 4, 5);
        Timed t(h, 3);
        hipLaunchKernelGGL((stage_kernel<CfgC, MFMA, false>), dim3((n_active + CfgC::B - 1) / CfgC::B), dim3(CfgC::NT), CfgC::LDS_BYTES, st, p);
    }
    {
        StageParams p{}; fill(p, h->d_xC, h->d_xD, 11, 6, 7);
        Timed t(h, 4);
        hipLaunchKernelGGL((stage_kernel<CfgD, MFMA, false>), dim3((n_active + CfgD::B - 1) / CfgD::B), dim3(CfgD::NT), CfgD::LDS_BYTES, st, p);
    }
    {
        StageParams p{}; fill(p, h->d_xD, nullptr, 15, 8, 9);
        p.hist19 = h->d_state[10]; p.w19 = h->d_conv[19]; p.feat = h->d_feat; p.emb = h->d_emb; p.nfeat = h->d_nfeat; p.TR = h->TR;
        p.dbg_off[4] = dbg_off[19];
        Timed t(h, 5);
        hipLaunchKernelGGL((stage_kernel<CfgE, MFMA, true>), dim3((n_active + CfgE::B - 1) / CfgE::B), dim3(CfgE::NT), CfgE::LDS_BYTES, st, p);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// one of stages B..E of the register-resident kernels (config CR; Timed class cls = 2..5), in the f16-split form (config CH, WG waves
// per workgroup) when HX: a launch whose workgroups are (nearly) alone on their CUs runs the three-slot weight ring (owwhip_hx.h
// WRing): same results
template <class CR, class CH, int WG, bool LAST, bool DBG, bool HX>
void launch_rstage(oww_ctx* h, const owr::RStageParams& p, int cls) {
    hipStream_t st = h->stream;
    Timed t(h, cls);
    const int nwg = (p.n_groups + WG - 1) / WG;
    if constexpr (HX && !DBG && std::is_same<CH, owh::HB>::value) {
        // stage B, no group list: weights resident in LDS, persistent workgroups that each walk a contiguous range of groups
        const bool resident = p.glist == nullptr && p.n_groups > 0 && (h->resident_b < 0 ? p.n_groups >= kResidentBMinGroups : h->resident_b != 0);
        if (resident) {
            const int grid = std::max(1, std::min(h->resident_b_wgs, (p.n_groups + owh::RES_B_WG - 1) / owh::RES_B_WG));
            hipLaunchKernelGGL((owh::hstage_kernel<CH, LAST, false, owh::RES_B_WG, 1>), dim3(grid), dim3(64 * owh::RES_B_WG), owh::RES_B_LDS_BYTES, st, p);
            return;
        }
    }
    if (HX && !DBG && nwg <= h->small_wgs) hipLaunchKernelGGL((owh::hstage_kernel<CH, LAST, false, WG, 3>), dim3(nwg), dim3(64 * WG), 0, st, p);
    else if (HX) hipLaunchKernelGGL((owh::hstage_kernel<CH, LAST, DBG, WG>), dim3(nwg), dim3(64 * WG), 0, st, p);
    else hipLaunchKernelGGL((owr::rstage_kernel<CR, LAST, DBG>), dim3((p.n_groups + 3) / 4), dim3(256), 0, st, p);
}

// register-resident kernels (owwhip_rr.h): every wave independent, groups of 1 / 1 / 2 / 4 / 8 streams per wave
template <bool DBG, bool HX>
int run_cnn_rr(oww_ctx* h, const StepArgs& a, int n_active, int mel_stride, int mel_off) {
    using namespace owr;
    hipStream_t st = h->stream;
    int off = 0, dbg_off[20];
    for (int l = 0; l < 20; ++l) { dbg_off[l] = off; off += kLayerOut[l][0] * kLayerOut[l][1] * kLayerOut[l][2]; }
    {
        RAParams p{};
        p.mel = a.mel ? a.mel : h->d_mel; p.mel_stride = mel_stride; p.mel_off = mel_off;
        p.hist_mel = h->d_state[0]; p.hist2 = h->d_state[1];
        p.w0 = h->d_conv[0]; p.w1 = h->d_conv[1]; p.w2 = h->d_conv[2];
        for (int i = 0; i < 3; ++i) { p.scale[i] = h->d_scale[i]; p.shift[i] = h->d_shift[i]; p.dbg_off[i] = dbg_off[i]; }
        p.xout = h->d_xA; p.n_streams = n_active; p.S = h->Spad;
        p.dbg = DBG ? h->d_dbg : nullptr; p.dbg_stride = DBG_FLOATS;
        for (int i = 0; i < 3; ++i) { p.clampv[i] = -0.4f * ldexpf(1.f, h->hx_e[i]); p.dbg_mul[i] = ldexpf(1.f, -h->hx_e[i]); }
        p.xmul = ldexpf(1.f, h->hx_xexp[0]);
        p.range_flag = HX ? h->d_range : nullptr;
        p.stream_on = a.on;
        const int grid = std::min((n_active + 3) / 4, 768);           // persistent: 3 workgroups of 4 waves per CU
        Timed t(h, 1);
        if (HX && a.fused_pcm) {
            // mel front end + stage A in one launch: PCM in, pooled stage-A activations out (BASELINE configs[2] "mel+embedding fused")
            owf::MelAParams q{};
            q.a = p; q.a.mel = nullptr; q.a.n_streams = h->S;          // the PCM buffer holds the S real streams only
            q.pcm = a.fused_pcm; q.tail = h->d_tail; q.nfeat = h->d_nfeat; q.hann = h->d_hann; q.mel_start = h->d_mstart; q.mel_taps = h->d_taps; q.mel_off = h->d_meloff; q.mel_dst = h->d_meldst;
            q.mel_out = h->cfg.debug_layers ? h->d_mel : nullptr;
            const int per_cu = std::max(1, std::min(12 / owf::FA_WG, 163840 / owf::FA_LDS_BYTES));     // persistent: 12 waves per CU
            const int g2 = std::max(1, std::min((q.a.n_streams + owf::FA_WG - 1) / owf::FA_WG, 256 * per_cu));
            hipLaunchKernelGGL(owf::hmelA_kernel<DBG>, dim3(g2), dim3(64 * owf::FA_WG), owf::FA_LDS_BYTES, st, q);
        }
        else if (HX) hipLaunchKernelGGL(owh::hstageA_kernel<DBG>, dim3(std::min((n_active + 3) / 4, 256 * OWH_WPS_A)), dim3(256), 0, st, p);
        else hipLaunchKernelGGL(rstageA_kernel<DBG>, dim3(grid), dim3(256), 0, st, p);
    }
    auto fill = [&](const float* xin, float* xout, int first_layer, int sb, int sd, int spt) {
        RStageParams p{};
        p.xin = xin; p.xout = xout; p.hist_b = h->d_state[sb]; p.hist_d = h->d_state[sd];
        for (int i = 0; i < 4; ++i) {
            p.w[i] = h->d_conv[first_layer + i]; p.scale[i] = h->d_scale[first_layer + i];
            p.shift[i] = h->d_shift[first_layer + i]; p.dbg_off[i] = dbg_off[first_layer + i];
            p.clampv[i] = -0.4f * ldexpf(1.f, h->hx_e[first_layer + i]); p.dbg_mul[i] = ldexpf(1.f, -h->hx_e[first_layer + i]);
        }
        p.dbg_mul[4] = ldexpf(1.f, -h->hx_e[19]);
        p.xmul = ldexpf(1.f, h->hx_xexp[first_layer / 4 + 1]);      // first_layer 3, 7, 11, 15 -> hand-over 1..4
        p.emb_mul = ldexpf(1.f, -h->hx_e[19]);
        p.n_groups = (n_active + spt - 1) / spt; p.S = h->Spad;
        p.dbg = DBG ? h->d_dbg : nullptr; p.dbg_stride = DBG_FLOATS;
        p.range_flag = HX ? h->d_range : nullptr;
        p.stream_on = a.on;
        if (HX && a.lists) {                                        // spt 1, 2, 4, 8 -> list 0, 1, 2, 3
            const int k = spt == 1 ? 0 : spt == 2 ? 1 : spt == 4 ? 2 : 3;
            p.glist = a.gl[k]; p.n_groups = a.gn[k];
        }
        return p;
    };
    launch_rstage<RB, owh::HB, OWH_WG_B, false, DBG, HX>(h, fill(h->d_xA, h->d_xB, 3, 2, 3, RB::SPT), 2);
    launch_rstage<RC, owh::HC, OWH_WG_C, false, DBG, HX>(h, fill(h->d_xB, h->d_xC, 7, 4, 5, RC::SPT), 3);
    launch_rstage<RD, owh::HD, OWH_WG_D, false, DBG, HX>(h, fill(h->d_xC, h->d_xD, 11, 6, 7, RD::SPT), 4);
    RStageParams pe = fill(h->d_xD, nullptr, 15, 8, 9, RE::SPT);
    pe.hist19 = h->d_state[10]; pe.w19 = h->d_conv[19]; pe.feat = h->d_feat; pe.emb = h->d_emb; pe.nfeat = h->d_nfeat; pe.TR = h->TR;
    pe.dbg_off[4] = dbg_off[19];
    launch_rstage<RE, owh::HE, OWH_WG_E, true, DBG, HX>(h, pe, 5);
    HIPCHK(hipGetLastError());
    return 0;
}

int run_cnn(oww_ctx* h, const StepArgs& a, int n_active, int mel_stride, int mel_off) {
    // grids cover whole workgroups of streams: round up to the largest per-workgroup stream count
    n_active = std::min(h->Spad, (n_active + 7) / 8 * 8);
    if (h->hx) return a.dbg ? run_cnn_rr<true, true>(h, a, n_active, mel_stride, mel_off) : run_cnn_rr<false, true>(h, a, n_active, mel_stride, mel_off);
    if (h->rr) return a.dbg ? run_cnn_rr<true, false>(h, a, n_active, mel_stride, mel_off) : run_cnn_rr<false, false>(h, a, n_active, mel_stride, mel_off);
    return h->mfma ? run_cnn_t<true>(h, a, n_active, mel_stride, mel_off) : run_cnn_t<false>(h, a, n_active, mel_stride, mel_off);
}

// what every post-processing launch site takes from the handle (owwhip_postproc.h): the rules of the fixed labels or of the bank's heads,
// and the streams' VAD gate
owq::Rules post_rules(const oww_ctx* h) { return {h->d_patience, h->d_threshold, h->debounce_frames}; }
owq::Rules bank_post_rules(const oww_ctx* h) { return {h->d_bank_pat, h->d_bank_thr, h->debounce_frames}; }
owq::Gate post_gate(const oww_ctx* h) { return {h->d_vadring, h->d_nvad, h->vad_threshold}; }

int heads_lds_bytes(int NH) { return (HD_SB * 100 + 2 * HD_SB * (NH + 4) + HD_SB * HD_MAXNETS) * 4; }

// heads over streams [0,n_active): ring mode (ext == nullptr) or external features
// heads_generic_kernel in the shape that fits the launch (owwhip_kernels.h): <4 streams per wave, 4 waves> below GH_BIG_STREAMS
// streams, <16, 2> from there on when no head is wider than 128 hidden units (its accumulator registers are sized for that:
// train.py's default width and the released multiclass models).  OWW_GENERIC_SPW=4|16 pins one -- tests run both on the same inputs.
// hs = LDS stride of a hidden vector.
void launch_generic_heads(oww_ctx* h, const HeadParams& p, int n_active, int nb, int ne, hipStream_t st) {
    const int hs = (std::max(h->generic_hmax, 1) + 3) & ~3;
    const bool big = h->generic_hmax <= 128 && (h->generic_spw == 16 || (h->generic_spw == 0 && n_active >= GH_BIG_STREAMS));
    if (big) hipLaunchKernelGGL((heads_generic_kernel<16, 2, 2>), dim3((n_active + 31) / 32), dim3(128), gh_lds_bytes(16, 2, hs), st, p, nb, ne, hs);
    else hipLaunchKernelGGL((heads_generic_kernel<4, 4>), dim3((n_active + 15) / 16), dim3(256), gh_lds_bytes(4, 4, hs), st, p, nb, ne, hs);
}

int run_heads(oww_ctx* h, const StepArgs& a, int n_active, bool accumulate_max, const float* ext, int only_head, float* raw_out, int force_generic) {
    hipStream_t st = h->stream;
    Timed t(h, 6);
    HeadParams base{};
    base.feat = ext ? ext : h->d_feat; base.ext = ext ? 1 : 0; base.TR = h->TR; base.nfeat = h->d_nfeat;
    base.raw = raw_out; base.NL = h->NL; base.S = n_active; base.accumulate_max = accumulate_max ? 1 : 0;
    base.stream_on = ext ? nullptr : a.on;
    const bool fast_ok = h->mfma && !force_generic;
    if (fast_ok) {
        for (auto& g : h->groups) {
            if (only_head >= 0) {
                bool has = false;
                for (int ni : g.nets) has |= h->nets[ni].head == only_head;
                if (!has) continue;
            }
            if (h->hx) {
                owh::HeadHxParams q{};
                q.feat = base.feat; q.ext = base.ext; q.TR = base.TR; q.T = g.T; q.nfeat = base.nfeat; q.w1hx = g.d_w1hx;
                q.raw = raw_out; q.NL = h->NL; q.S = n_active; q.accumulate_max = base.accumulate_max;
                q.range_flag = h->d_range; q.stream_on = a.on;
                if (a.lists && !ext) { q.ids = a.gl[0]; q.n_ids = a.gn[0]; }
                const int n_pos = q.ids ? q.n_ids : q.S;
                if (a.post_in_heads) {
                    owh::HeadHxPost& pp = q.post;
                    pp.enabled = 1; pp.scores = h->d_scores; pp.ring = h->d_ring; pp.npred = h->d_npred; pp.nfeat = h->d_nfeat;
                    pp.rules = post_rules(h); pp.gate = post_gate(h);
                }
                for (int i = 0; i < g.n_nets; ++i) q.net[i] = g.hx_net[i];
                q.fscale = std::ldexp(1.0f, h->hx_efeat);
                const dim3 grid((n_pos + 32 * owh::HX_WG - 1) / (32 * owh::HX_WG)), block(64 * owh::HX_WG);
                // a launch that leaves workgroups alone on their CUs runs the deep weight ring (owwhip_hx.h: HX_NBUF_DEEP); same results
                const bool deep = (int)grid.x <= h->small_wgs_heads;
                const int nn = std::min(g.n_nets, 4);
                const int lds = 0;                                  // (the ring slots are static LDS objects: owwhip_hx.h hslot)
                if (g.ht == 8) {                                    // wide nets (<= 128 hidden units, <= 8 outputs): one or two per launch
                    if (nn == 1 && !deep) hipLaunchKernelGGL((owh::heads_hx_kernel<1, owh::HX_NBUF, owh::HX_WG, 8>), grid, block, lds, st, q);
                    else if (nn == 1) hipLaunchKernelGGL((owh::heads_hx_kernel<1, owh::HeadsDeep<2>::NBUF, owh::HX_WG, 8>), grid, block, lds, st, q);
                    else if (!deep) hipLaunchKernelGGL((owh::heads_hx_kernel<2, owh::HX_NBUF, owh::HX_WG, 8>), grid, block, lds, st, q);
                    else hipLaunchKernelGGL((owh::heads_hx_kernel<2, owh::HeadsDeep<4>::NBUF, owh::HX_WG, 8>), grid, block, lds, st, q);
                    continue;
                }
                switch (nn * 2 + (deep ? 1 : 0)) {
                    case 2: hipLaunchKernelGGL(owh::heads_hx_kernel<1>, grid, block, lds, st, q); break;
                    case 3: hipLaunchKernelGGL((owh::heads_hx_kernel<1, owh::HeadsDeep<1>::NBUF>), grid, block, lds, st, q); break;
                    case 4: hipLaunchKernelGGL(owh::heads_hx_kernel<2>, grid, block, lds, st, q); break;
                    case 5: hipLaunchKernelGGL((owh::heads_hx_kernel<2, owh::HeadsDeep<2>::NBUF>), grid, block, lds, st, q); break;
                    case 6: hipLaunchKernelGGL(owh::heads_hx_kernel<3>, grid, block, lds, st, q); break;
                    case 7: hipLaunchKernelGGL((owh::heads_hx_kernel<3, owh::HeadsDeep<3>::NBUF>), grid, block, lds, st, q); break;
                    case 8: hipLaunchKernelGGL(owh::heads_hx_kernel<4>, grid, block, lds, st, q); break;
                    default: hipLaunchKernelGGL((owh::heads_hx_kernel<4, owh::HeadsDeep<4>::NBUF>), grid, block, lds, st, q); break;
                }
                continue;
            }
            HeadParams p = base;
            p.nets = g.d_nets; p.n_nets = g.n_nets; p.T = g.T; p.NH = g.NH; p.w1pk = g.d_w1pk; p.b1cat = g.d_b1cat;
            hipLaunchKernelGGL(heads64_kernel, dim3((n_active + HD_SB - 1) / HD_SB), dim3(HD_NT), heads_lds_bytes(g.NH), st, p);
        }
    }
    // generic kernel: nets that have no fast group, or everything when the fast path is off
    if (!fast_ok) {
        HeadParams p = base;
        p.nets = h->d_allnets; p.n_nets = (int)h->nets.size();
        int nb = 0, ne = (int)h->nets.size();
        if (only_head >= 0) { nb = h->head_nets[only_head].first; ne = h->head_nets[only_head].second; }
        launch_generic_heads(h, p, n_active, nb, ne, st);
    } else if (!h->generic_nets.empty()) {
        for (size_t hi = 0; hi < h->heads.size(); ++hi) {
            if (only_head >= 0 && (int)hi != only_head) continue;
            const int nb = h->head_nets[hi].first, ne = h->head_nets[hi].second;
            if (std::find(h->generic_nets.begin(), h->generic_nets.end(), nb) == h->generic_nets.end()) continue;
            HeadParams p = base;
            p.nets = h->d_allnets; p.n_nets = (int)h->nets.size();
            launch_generic_heads(h, p, n_active, nb, ne, st);
        }
    }
    // recurrent heads (model_type "rnn"): the same kernel in every family
    for (int ni : h->rnn_nets) {
        if (only_head >= 0 && h->nets[ni].head != only_head) continue;
        HeadParams p = base;
        p.nets = h->d_allnets; p.n_nets = (int)h->nets.size();
        hipLaunchKernelGGL((heads_rnn_kernel<RNN_SPW>), dim3((n_active + RNN_SPW - 1) / RNN_SPW), dim3(64), rnn_lds_bytes(h->nets[ni].T), st, p, ni);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

int launch_mel(oww_ctx* h, const StepArgs& a, const int16_t* d_pcm, int n_streams, int n_samples, int n_frames, int streaming, float* out,
               float* smax, int pcm_stride = 0, int max_only = 0, const float* floor_max = nullptr) {
    MelParams p{};
    p.pcm = d_pcm; p.n_samples = n_samples; p.n_frames = n_frames; p.streaming = streaming;
    p.pcm_stride = pcm_stride; p.max_only = max_only; p.floor_max = floor_max;
    p.tail = h->d_tail; p.nfeat = h->d_nfeat; p.out = out; p.smax = smax;
    p.hann = h->d_hann; p.mel_start = h->d_mstart; p.mel_taps = h->d_taps; p.S = n_streams;
    p.stream_on = streaming ? a.on : nullptr;
#ifndef OWK_MEL_WGS
#define OWK_MEL_WGS 6      // mel workgroups per CU in the persistent grid (20 KB LDS, 68 VGPRs each; 7 and 8 measured slower: 0.85 / 0.77 vs 0.73 ms)
#endif
    const int grid = std::min(n_streams, 256 * OWK_MEL_WGS);
    Timed t(h, 0);
    hipLaunchKernelGGL(mel_kernel, dim3(grid), dim3(MEL_NT), 0, h->stream, p);
    HIPCHK(hipGetLastError());
    return 0;
}

int do_reset(oww_ctx* h, const int* d_ids, int n, const float* d_featinit) {
    ResetParams p{};
    p.ids = d_ids; p.n = n; p.n_arrays = N_STATE;
    for (int a = 0; a < N_STATE; ++a) {
        p.dst[a] = h->d_state[a]; p.tmpl[a] = h->d_tmpl[a]; p.len[a] = h->state_len[a];
        p.spg[a] = h->rr ? kStateSpgRr[a] : 1; p.fpos[a] = h->rr ? kStateFposRr[a] : 16;
    }
    p.interleaved = h->hx && owh::kInterleave;
    p.tail = h->d_tail; p.nfeat = h->d_nfeat; p.npred = h->d_npred;
    p.ring = h->d_ring; p.ring_len = h->NL * OWW_SCORE_RING;
    p.feat = h->d_feat; p.feat_len = h->TR * OWW_EMB_DIM; p.feat_init = d_featinit;
    hipLaunchKernelGGL(reset_kernel, dim3(n), dim3(256), 0, h->stream, p);
    HIPCHK(hipGetLastError());
    return 0;
}

// one-shot allocation of max(n, 1) elements, zero-filled unless told otherwise
template <class T>
int dalloc(hipStream_t st, DevBuf<T>& b, size_t n, bool zero = true, int line = __builtin_LINE()) {
    HIPCHK(herr(b.alloc(n, line)));
    // the zero fill runs ON THE HANDLE'S STREAM: ordered in front of every kernel the handle will launch on it (its other streams are
    // forked from it by events), and no host round trip per buffer -- a legacy-stream fill would need one, because nothing orders
    // the handle's non-blocking streams behind the legacy stream (round 4: ~90 synchronisations per handle creation)
    if (zero) HIPCHK(hipMemsetAsync(b, 0, b.capacity() * sizeof(T), st));
    return 0;
}

// The one growth rule of the handle's scratch buffers.  n elements fit: nothing happens, no synchronisation (every hot-path call).
// Otherwise the handle's stream is drained -- queued work may still read the old block; hipFree would wait for it as well, this says
// so -- and the buffer becomes exactly n elements, contents not kept; on failure it is empty.  The caller words the error.
template <class T>
hipError_t grow(oww_ctx* h, DevBuf<T>& b, size_t n, int line = __builtin_LINE()) {
    if (n <= b.capacity()) return hipSuccess;
    const hipError_t e = hipStreamSynchronize(h->stream);
    return e != hipSuccess ? e : herr(b.reserve(n, line));
}

// ---- RCCL (librccl.so: ncclSend / ncclRecv over xGMI), bound at run time: the library is only needed by callers that shard streams
//      over GPUs WITHOUT torch.distributed (oww_comm_init / oww_gather_scores); nothing else in libowwhip touches it
struct RcclId { char b[128]; };           // ncclUniqueId (passed BY VALUE to ncclCommInitRank)
struct Rccl {
    void* lib = nullptr;
    int (*GetUniqueId)(void*) = nullptr;
    int (*CommInitRank)(void**, int, RcclId, int) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    int (*CommCount)(void*, int*) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    int (*Send)(const void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*Recv)(void*, size_t, int, int, void*, hipStream_t) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
};
Rccl g_rccl;
int rccl_load() {
    if (g_rccl.lib) return 0;
    void* lib = nullptr;
    // a copy the process already holds (torch bundles one) wins: two RCCL instances in one process is asking for trouble
    for (const char* name : {"librccl.so.1", "librccl.so"}) if (!lib) lib = dlopen(name, RTLD_NOW | RTLD_NOLOAD);
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) if (!lib) lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
    if (!lib) return fail(OWW_ESTATE, "librccl.so could not be loaded: %s", dlerror());
    Rccl r; r.lib = lib;
    bool ok = true;
    auto sym = [&](const char* n) { void* p = dlsym(lib, n); ok = ok && p != nullptr; return p; };
    r.GetUniqueId = reinterpret_cast<decltype(r.GetUniqueId)>(sym("ncclGetUniqueId"));
    r.CommInitRank = reinterpret_cast<decltype(r.CommInitRank)>(sym("ncclCommInitRank"));
    r.CommDestroy = reinterpret_cast<decltype(r.CommDestroy)>(sym("ncclCommDestroy"));
    r.CommCount = reinterpret_cast<decltype(r.CommCount)>(sym("ncclCommCount"));
    r.GroupStart = reinterpret_cast<decltype(r.GroupStart)>(sym("ncclGroupStart"));
    r.GroupEnd = reinterpret_cast<decltype(r.GroupEnd)>(sym("ncclGroupEnd"));
    r.Send = reinterpret_cast<decltype(r.Send)>(sym("ncclSend"));
    r.Recv = reinterpret_cast<decltype(r.Recv)>(sym("ncclRecv"));
    r.GetErrorString = reinterpret_cast<decltype(r.GetErrorString)>(sym("ncclGetErrorString"));
    if (!ok) return fail(OWW_ESTATE, "librccl.so lacks one of ncclGetUniqueId / ncclCommInitRank / ncclSend / ncclRecv / ncclGroupStart / ncclGroupEnd");
    g_rccl = r;
    return 0;
}
#define RCCLCHK(expr)                                                                                         \
    do {                                                                                                      \
        int e__ = (expr);                                                                                     \
        if (e__ != 0) return fail(OWW_EHIP, "%s failed: %s", #expr, g_rccl.GetErrorString ? g_rccl.GetErrorString(e__) : "?"); \
    } while (0)
void comm_release(oww_ctx* h);

// ---- head bank: the routed heads launch (one per width class that has subscribers) and its post-processing
bool bank_active(const oww_ctx* h) { return !h->bank_rt.tiles.empty(); }

void launch_bank_tiles(oww_ctx* h, owh::BankParams q, int c, int tile0, int ntiles) {
    q.tiles = h->d_bank_tiles + tile0;
    const dim3 grid(ntiles), block(64 * h->bank_rt.wg[c]);
    if (c == 0) {
        if (h->bank_rt.wg[c] == 4) hipLaunchKernelGGL((owh::heads_bank_kernel<4, 4>), grid, block, 0, h->stream, q);
        else hipLaunchKernelGGL((owh::heads_bank_kernel<1, 4>), grid, block, 0, h->stream, q);
    } else {
        if (h->bank_rt.wg[c] == 4) hipLaunchKernelGGL((owh::heads_bank_kernel<4, 8>), grid, block, 0, h->stream, q);
        else hipLaunchKernelGGL((owh::heads_bank_kernel<1, 8>), grid, block, 0, h->stream, q);
    }
}

int run_bank(oww_ctx* h, const StepArgs& a, bool accumulate_max) {
    owh::BankParams q{};
    q.feat = h->d_feat; q.ext = 0; q.TR = h->TR; q.nfeat = h->d_nfeat;
    q.entries = h->d_bank_entries; q.heads = h->d_bank_heads; q.K = h->bank_K;
    q.raw = h->d_bank_raw; q.accumulate_max = accumulate_max ? 1 : 0; q.range_flag = h->d_range; q.stream_on = a.on;
    q.fscale = std::ldexp(1.0f, h->hx_efeat);
    for (int c = 0; c < 2; ++c) {
        if (!h->bank_rt.ntiles[c]) continue;
#if OWH_BANK_PER_HEAD
        for (const auto& [t0, nt] : h->bank_rt.head_tiles[c]) { Timed t(h, 6); launch_bank_tiles(h, q, c, t0, nt); }   // (d) of tools/bench_head_bank.py
#else
        Timed t(h, 6);
        launch_bank_tiles(h, q, c, h->bank_rt.tile0[c], h->bank_rt.ntiles[c]);
#endif
    }
    HIPCHK(hipGetLastError());
    return 0;
}

int launch_bank_post(oww_ctx* h, const StepArgs& a) {
    if (!bank_active(h)) return 0;
    owh::BankPostParams pp{};
    pp.raw = h->d_bank_raw; pp.scores = h->d_bank_scores; pp.ring = h->d_bank_ring; pp.npred = h->d_bank_npred; pp.sub = h->d_bank_sub;
    pp.S = h->S; pp.K = h->bank_K;
    pp.rules = bank_post_rules(h); pp.gate = post_gate(h); pp.stream_on = a.on;
    {
        Timed t(h, 7);
        hipLaunchKernelGGL(owh::bank_post_kernel, dim3((h->S * h->bank_K + 255) / 256), dim3(256), 0, h->stream, pp);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- per-stream verifiers: with any per-stream assignment, stream_verifier_kernel verifies every (stream, column / slot) pair that
//      has a verifier -- its pool verifier or the column's handle-wide one -- and verifier_kernel does not run
bool sv_active(const oww_ctx* h) { return h->vasg_n > 0; }

int launch_stream_verifiers(oww_ctx* h, const StepArgs& a) {
    HIPCHK(hipMemsetAsync(h->d_sv_eval, 0, sizeof(unsigned long long), h->stream));
    if (h->sv_n == 0) return 0;
    StreamVerifierParams v{};
    v.list = h->d_svlist; v.n = h->sv_n;
    v.raw = h->d_raw; v.bank_raw = h->d_bank_raw; v.NL = h->NL; v.K = h->bank_K;
    v.feat = h->d_feat; v.nfeat = h->d_nfeat; v.TR = h->TR;
    v.pool_w = h->d_vpool_w; v.pool_b = h->d_vpool_b; v.pool_stride = h->vpool_stride;
    v.ver_w = h->d_verw; v.ver_b = h->d_verb; v.ver_stride = h->ver_stride;
    v.stream_on = a.on; v.n_eval = h->d_sv_eval;
    const int per_block = 4 * SV_PAIRS;
    hipLaunchKernelGGL(stream_verifier_kernel, dim3((h->sv_n + per_block - 1) / per_block), dim3(256), 0, h->stream, v);
    HIPCHK(hipGetLastError());
    return 0;
}

// one chunk of the streaming step on device-resident mel rows
// (k, c: the mel rows of this chunk sit at row 8c of 8k per stream; first / last: of the CALL, which may span several mel slices)
int step_chunk(oww_ctx* h, const StepArgs& a, int k, int c, bool first, bool last) {
    if (int rc = run_cnn(h, a, h->Spad, 8 * k * 32, c * 8 * 32)) return rc;
    // the bank reads this chunk's ring rows before the fixed heads launch (which may advance the ring counters: post_in_heads)
    if (bank_active(h)) if (int rc = run_bank(h, a, !first)) return rc;
    if (int rc = run_heads(h, a, h->Spad, !first, nullptr, -1, h->d_raw, 0)) return rc;
    if (sv_active(h) && last) {                      // (as below: after the maximum over the call's chunks, before the ring advances)
        if (int rc = launch_stream_verifiers(h, a)) return rc;
    } else if (h->n_verifiers > 0 && last) {         // after the maximum over the call's chunks, on the newest feature rows
        VerifierParams v{};
        v.raw = h->d_raw; v.feat = h->d_feat; v.nfeat = h->d_nfeat; v.w = h->d_verw; v.bias = h->d_verb; v.thr = h->d_verthr; v.T = h->d_verT;
        v.wstride = h->ver_stride; v.NL = h->NL; v.TR = h->TR; v.S = h->S; v.stream_on = a.on;
        hipLaunchKernelGGL(verifier_kernel, dim3((h->S + 3) / 4), dim3(256), 0, h->stream, v);
    }
    if (!a.post_in_heads)
        hipLaunchKernelGGL(advance_kernel, dim3((h->Spad + 255) / 256), dim3(256), 0, h->stream, h->d_nfeat, h->Spad, a.on);
    return 0;
}

// voice-activity stand-in network for this step's 1280 new samples of every stream -> one score per stream into the VAD ring
int launch_vad(oww_ctx* h, const StepArgs& a, const int16_t* d_pcm, int n_samples) {
    const int G = (h->S + 15) / 16;
    {
        owv::VadFrontParams p{};
        p.pcm = d_pcm; p.n_samples = n_samples; p.S = h->S; p.hann = h->d_vad_hann; p.mag_gain = h->vad_gain;
        p.w = h->d_vad_encw; p.bias = h->d_vad_encb; p.xout = h->d_vadx; p.range_flag = h->d_range; p.stream_on = a.on;
        const int grid = std::min((h->S + owv::V_WG - 1) / owv::V_WG, 256);          // persistent: one 8-wave workgroup per CU
        Timed t(h, 8);
        hipLaunchKernelGGL(owv::vad_front_kernel, dim3(grid), dim3(64 * owv::V_WG), owv::V_LDS_BYTES, h->stream, p);
    }
    {
        owv::VadLstmParams p{};
        p.xin = h->d_vadx; p.hc = h->d_vadhc; p.w = h->d_vad_lstmw; p.bias = h->d_vad_lstmb; p.wd = h->d_vad_wd; p.bd = h->vad_bd;
        p.ring = h->d_vadring; p.n_vad = h->d_nvad; p.last = h->d_vadlast; p.S = h->S; p.n_groups = G; p.stream_on = a.on;
        p.range_flag = h->d_range;
        if (a.lists) { p.glist = a.gl[4]; p.n_groups = a.gn[4]; }
        Timed t(h, 9);
        hipLaunchKernelGGL(owv::vad_lstm_kernel, dim3((p.n_groups + owv::L_WG - 1) / owv::L_WG), dim3(64 * owv::L_WG), 0, h->stream, p);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// Lists for a masked step with few participants (owwhip_masked_host.h): [stream ids | C groups | D groups | E groups | VAD groups] built
// straight into one pinned staging buffer, copied to the device on the compute stream (ordered before the step's kernels), and entered
// into a (lists, gl, gn).  Returns the number of participants, -1 when the dense launches should be used, or an OWW_E* code - 100 on
// failure.  Only a return > 0 fills a.
int build_active_lists(oww_ctx* h, const uint8_t* on, StepArgs& a) {
    const int S = h->S, n_act = owl::participants(on, S);
    if (n_act <= 0) return n_act;
    if (!h->hx || !h->fuse || !h->generic_nets.empty() || !h->rnn_nets.empty()) return -1;       // the group lists are read by the default family's launches only
    const size_t need = owl::lists_capacity(S);
    if (grow(h, h->d_lists, need) != hipSuccess) return fail(OWW_ENOMEM, "oww_step_masked: out of device memory") - 100;
    for (int i = 0; i < 2; ++i) {
        if (need > h->h_lists[i].capacity()) {                    // (its own double buffering: the copy that read the old block has run)
            if (h->lists_ev[i]) (void)hipEventSynchronize(h->lists_ev[i]);
            if (h->h_lists[i].reserve(need, hipHostMallocDefault)) return fail(OWW_ENOMEM, "oww_step_masked: out of page-locked memory") - 100;
        }
        if (!h->lists_ev[i] && h->lists_ev[i].create(hipEventDisableTiming)) return fail(OWW_EHIP, "hipEventCreate failed") - 100;
    }
    const unsigned turn = h->lists_turn++ & 1u;
    (void)hipEventSynchronize(h->lists_ev[turn]);              // the copy that last read this staging buffer has run
    int* out = h->h_lists[turn];
    size_t off[5];
    owl::build_lists(on, S, out, a.gn, off);
    for (int k = 0; k < 5; ++k) a.gl[k] = h->d_lists + off[k];
    const size_t total = off[4] + (size_t)a.gn[4];              // (> 0: somebody takes part)
    if (copy_async(h->d_lists, out, total * sizeof(int), hipMemcpyHostToDevice, h->stream) != hipSuccess) return fail(OWW_EHIP, "oww_step_masked: list upload failed") - 100;
    (void)hipEventRecord(h->lists_ev[turn], h->stream);
    a.lists = true;
    return n_act;
}

int launch_postproc(oww_ctx* h, const StepArgs& a);
int launch_step(oww_ctx* h, const StepArgs& args, const int16_t* d_pcm, int k) {
    if (h->vad) {
        if (k != 1) return fail(OWW_EINVAL, "with the on-device VAD network a step carries exactly one 1280-sample chunk per stream (got %d)", k);
        if (int rc = launch_vad(h, args, d_pcm, OWW_CHUNK * k)) return rc;
    }
    StepArgs a = args;
    a.post_in_heads = h->post_in_heads && k == 1 && h->n_verifiers == 0 && !sv_active(h);
    if (h->fuse && k == 1 && (reinterpret_cast<uintptr_t>(d_pcm) & 15) == 0) {      // (the fused front end uses 16-byte sample loads)
        a.fused_pcm = d_pcm;
        if (int rc = step_chunk(h, a, 1, 0, true, true)) return rc;
    } else {
        if (int rc = launch_mel(h, a, d_pcm, h->S, OWW_CHUNK * k, 8 * k, 1, h->d_mel, nullptr)) return rc;
        for (int c = 0; c < k; ++c)
            if (int rc = step_chunk(h, a, k, c, c == 0, c == k - 1)) return rc;
    }
    if (a.post_in_heads) { HIPCHK(hipGetLastError()); return launch_bank_post(h, a); }      // post-processing already ran inside the heads launch
    if (int rc = launch_postproc(h, a)) return rc;
    return launch_bank_post(h, a);
}

// A call of more chunks than the handle's mel buffer holds (n_chunks > max_chunks; the reference takes any length: model.py:287-298,
// utils.py:387-401).  The reference runs its melspectrogram graph ONCE over the call, so the clamp floor "maximum - 80 dB" is the
// call's; evaluating the call in slices of max_chunks chunks with each slice's own maximum would move the floor (a quiet start of a
// call whose loud part comes later).  Two passes: the mel kernel over the whole call for its per-stream maximum only, then the
// slices -- mel rows with that shared floor, one embedding and one heads evaluation per chunk, raw scores max-combined over ALL
// chunks of the call -- and one post-processing pass.  d_pcm: [S][1280 K] on the device.
int launch_step_long(oww_ctx* h, const StepArgs& a, const int16_t* d_pcm, int K) {
    if (h->vad) return fail(OWW_EINVAL, "with the on-device VAD network a step carries exactly one 1280-sample chunk per stream (got %d)", K);
    if (!h->d_callmax) if (int rc = dalloc(h->stream, h->d_callmax, (size_t)h->Spad)) return rc;
    if (int rc = launch_mel(h, a, d_pcm, h->S, OWW_CHUNK * K, 8 * K, 1, nullptr, h->d_callmax, 0, 1, nullptr)) return rc;
    for (int o = 0; o < K; o += h->kmax) {
        const int ks = std::min(h->kmax, K - o);
        if (int rc = launch_mel(h, a, d_pcm + (size_t)o * OWW_CHUNK, h->S, OWW_CHUNK * ks, 8 * ks, 1, h->d_mel, nullptr, OWW_CHUNK * K, 0, h->d_callmax)) return rc;
        for (int c = 0; c < ks; ++c)
            if (int rc = step_chunk(h, a, ks, c, o + c == 0, o + c == K - 1)) return rc;
        h->k_last = ks;
    }
    if (int rc = launch_postproc(h, a)) return rc;
    return launch_bank_post(h, a);
}

int launch_postproc(oww_ctx* h, const StepArgs& a) {
    PostParams pp{};
    pp.raw = h->d_raw; pp.scores = h->d_scores; pp.ring = h->d_ring; pp.npred = h->d_npred;
    pp.NL = h->NL; pp.S = h->Spad;
    pp.rules = post_rules(h); pp.gate = post_gate(h); pp.stream_on = a.on;
    {
        Timed t(h, 7);
        hipLaunchKernelGGL(postproc_kernel, dim3((h->Spad + 127) / 128), dim3(128), 0, h->stream, pp);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- detection events (oww_events_*; kernels in owwhip_events.h).  Not part of launch_step, hence of no captured graph: the entry
//      points call launch_events behind the step's launches and before the score copy, on handles that configured events only.
bool events_on(const oww_ctx* h) { return h->evt_cap > 0; }

// device buffers of one set: records and snapshots with one spare entry behind the capacity (never written), counts zeroed
int alloc_event_buf(oww_ctx* h, oww_ctx::EventBuf& b, bool host_mirror) {
    if (int rc = dalloc(h->stream, b.d_rec, (size_t)h->evt_cap + 1)) return rc;
    if (int rc = dalloc(h->stream, b.d_count, 2)) return rc;
    if (h->evt_rows > 0) if (int rc = dalloc(h->stream, b.d_snap, ((size_t)h->evt_cap + 1) * h->evt_rows * OWW_EMB_DIM, false)) return rc;
    if (h->aud_evt > 0) {
        const uint64_t nb = owa::snapshot_bytes(h->evt_cap, h->aud_evt);
        if (b.d_asnap.alloc((size_t)(nb / sizeof(int16_t))))
            return fail(OWW_ENOMEM, "oww_audio_configure: out of device memory for %llu bytes of event audio snapshots", (unsigned long long)nb);
    }
    if (host_mirror) {
        HIPCHK(herr(b.h_rec.alloc((size_t)h->evt_cap, hipHostMallocDefault)));
        HIPCHK(herr(b.h_count.alloc(2, hipHostMallocDefault)));
        b.h_count[0] = b.h_count[1] = 0;
    }
    return 0;
}

int alloc_events(oww_ctx* h) {
    const long long pairs = (long long)h->S * (h->NL + h->bank_K);
    if (pairs > 0x7fffffffLL - owe::EV_WG) return fail(OWW_EINVAL, "oww_events_configure: %lld (stream, column) pairs are more than the event kernels index", pairs);
    h->evt_blocks = (int)((pairs + owe::EV_WG - 1) / owe::EV_WG);
    if (int rc = dalloc(h->stream, h->d_evblock, (size_t)std::max(h->evt_blocks, 1))) return rc;
    if (int rc = dalloc(h->stream, h->d_evt_thr, (size_t)std::max(h->NL, 1), false)) return rc;
    std::vector<float> half(std::max(h->NL, 1), 0.5f);
    HIPCHK(copy_async(h->d_evt_thr, half.data(), half.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
    if (int rc = alloc_event_buf(h, h->evt_sync, false)) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

// The events of the call whose launches were just enqueued, into `buf`.  any_on = false: a masked call nobody takes part in.
int launch_events(oww_ctx* h, const StepArgs& a, const oww_ctx::EventBuf& buf, bool any_on = true) {
    if (!any_on || h->evt_blocks == 0) {
        HIPCHK(hipMemsetAsync(buf.d_count, 0, 2 * sizeof(int), h->stream));
        return 0;
    }
    owe::EventsParams p{};
    p.scores = h->d_scores; p.bank_scores = h->d_bank_scores; p.bank_sub = h->d_bank_sub;
    p.thr_fixed = h->d_evt_thr; p.thr_bank = h->evt_bank_thr; p.stream_on = a.on;
    p.npred = h->d_npred; p.nfeat = h->d_nfeat; p.feat = h->d_feat;
    p.TR = h->TR; p.NL = h->NL; p.K = h->bank_K;
    p.n_pairs = h->S * (h->NL + h->bank_K); p.n_blocks = h->evt_blocks; p.block_count = h->d_evblock;
    p.rec = buf.d_rec; p.count = buf.d_count; p.snap = buf.d_snap; p.capacity = h->evt_cap; p.rows = h->evt_rows;
    {
        Timed t(h, 7);
        hipLaunchKernelGGL(owe::events_count_kernel, dim3(h->evt_blocks), dim3(owe::EV_WG), 0, h->stream, p);
    }
    {
        Timed t(h, 7);
        hipLaunchKernelGGL(owe::events_write_kernel, dim3(h->evt_blocks), dim3(owe::EV_WG), 0, h->stream, p);
    }
    if (h->aud_evt > 0) {                        // the stored records' audio: the ring already holds the detecting chunk (launch_audio_append)
        owa::EventsAudioParams q{};
        q.count = buf.d_count; q.rec = buf.d_rec; q.ring = h->d_aring; q.counter = h->d_acount; q.snap = buf.d_asnap;
        q.S = h->S; q.capacity = h->evt_cap; q.event_chunks = (uint32_t)h->aud_evt; q.ring_chunks = (uint32_t)h->aud_ring;
        const long long waves = (long long)h->evt_cap * h->aud_evt;           // the most chunk copies a call can have
        const int grid = (int)std::min<long long>(owa::AU_EVENT_WGS, (waves + owa::AU_WG / 64 - 1) / (owa::AU_WG / 64));
        Timed t(h, 7);
        hipLaunchKernelGGL(owa::events_audio_kernel, dim3(grid), dim3(owa::AU_WG), 0, h->stream, q);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- per-stream audio rings (oww_audio_configure; kernels in owwhip_audio.h, arithmetic in owwhip_audio_host.h).  Like events not
//      part of launch_step, hence of no captured graph and of no borrowed-stream entry (oww_embed, oww_embed_clips, oww_mel, the commit
//      probes): the entry points that advance streams call launch_audio_append where they call launch_events, in front of it.
bool audio_on(const oww_ctx* h) { return h->aud_ring > 0; }

int alloc_audio(oww_ctx* h) {
    const uint64_t nb = owa::ring_bytes(h->S, h->aud_ring);
    if (nb / sizeof(int16_t) > (uint64_t)SIZE_MAX / sizeof(int16_t) || h->d_aring.alloc((size_t)(nb / sizeof(int16_t))))
        return fail(OWW_ENOMEM, "oww_audio_configure: out of device memory for %llu bytes of audio rings (%d streams x %d chunks x %llu)",
                    (unsigned long long)nb, h->S, h->aud_ring, (unsigned long long)owa::kChunkBytes);
    if (h->d_acount.alloc((size_t)h->S))
        return fail(OWW_ENOMEM, "oww_audio_configure: out of device memory for %llu bytes of chunk counters", (unsigned long long)owa::counter_bytes(h->S));
    HIPCHK(hipMemsetAsync(h->d_aring, 0, (size_t)nb, h->stream));
    HIPCHK(hipMemsetAsync(h->d_acount, 0, (size_t)owa::counter_bytes(h->S), h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

// The call's k chunks per stream, [S][k * 1280] at d_src (any 2-byte alignment), into the rings of the streams that took part, behind
// the step's launches on the handle's stream.  d_src = nullptr: zero the rings and counters of ids[n] (nullptr: of every stream).
int launch_audio_append(oww_ctx* h, const StepArgs& a, const int16_t* d_src, int k, bool any_on = true) {
    if (!any_on) return 0;
    owa::AppendParams p{};
    p.src = d_src; p.ring = h->d_aring; p.counter = h->d_acount; p.stream_on = a.on;
    p.ids = a.lists ? a.gl[0] : nullptr; p.n = a.lists ? a.gn[0] : h->S;
    p.S = h->S; p.k = (uint32_t)k; p.ring_chunks = (uint32_t)h->aud_ring;
    if (p.n <= 0) return 0;
    const dim3 grid((p.n + owa::AU_WG / 64 - 1) / (owa::AU_WG / 64));
    {
        Timed t(h, 7);
        if (reinterpret_cast<uintptr_t>(d_src) & 15) hipLaunchKernelGGL(owa::audio_append_kernel<false>, grid, dim3(owa::AU_WG), 0, h->stream, p);
        else hipLaunchKernelGGL(owa::audio_append_kernel<true>, grid, dim3(owa::AU_WG), 0, h->stream, p);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

int audio_reset(oww_ctx* h, const int* d_ids, int n) {
    owa::AppendParams p{};
    p.ring = h->d_aring; p.counter = h->d_acount; p.ids = d_ids; p.n = d_ids ? n : h->S;
    p.S = h->S; p.ring_chunks = (uint32_t)h->aud_ring;
    hipLaunchKernelGGL(owa::audio_append_kernel<true>, dim3((p.n + owa::AU_WG / 64 - 1) / (owa::AU_WG / 64)), dim3(owa::AU_WG), 0, h->stream, p);
    HIPCHK(hipGetLastError());
    return 0;
}

// sticky out-of-range flag of the f16-split kernels (owwhip_hx.h nan_guard): read straight from the mapped host word
int range_check(oww_ctx* h, const char* where) {
    if (h->h_range && *(volatile int*)h->h_range)
        return fail(OWW_ERANGE, "%s: an activation left the f16 range of the fp16-split kernels (use_mfma = 3) -- scores since then are not "
                    "trustworthy; create the handle with use_mfma = 1 (exact fp32) for these weights, or clear with oww_range_status(h, 1)", where);
    return 0;
}

// oww_embed / oww_embed_clips borrow the streaming machinery of the first streams: their state (conv histories, feature ring
// rows, frame counters) is parked in a scratch buffer for the duration of the call and put back afterwards
int park_state(oww_ctx* h, int n_streams, bool save) {
    const size_t n8 = std::min<size_t>(h->Spad, ((size_t)n_streams + 7) / 8 * 8);
    size_t need = h->Spad + n8 * (size_t)h->TR * 96;
    for (int a = 0; a < N_STATE; ++a) need += n8 * (size_t)h->state_len[a];
    if (save && grow(h, h->d_save, need) != hipSuccess) return fail(OWW_ENOMEM, "out of device memory for %zu parked state bytes", need * sizeof(float));
    if (need > h->d_save.capacity()) return fail(OWW_ESTATE, "park_state: nothing parked");
    float* q = h->d_save;
    auto cp = [&](void* live, size_t nfl) -> int {
        HIPCHK(copy_async(save ? (void*)q : live, save ? live : (void*)q, nfl * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
        q += nfl;
        return 0;
    };
    for (int a = 0; a < N_STATE; ++a) if (int rc = cp(h->d_state[a], n8 * (size_t)h->state_len[a])) return rc;
    if (int rc = cp(h->d_feat, n8 * (size_t)h->TR * 96)) return rc;
    if (int rc = cp(h->d_nfeat, h->Spad)) return rc;         // the frame counters of EVERY stream advance with the borrowed steps
    return 0;
}

// OWW_COMMIT_TIMING=1: wall-clock of the phases of oww_commit on stderr (development aid; handle creation should stay in the tens of
// milliseconds -- the reference constructs Model objects freely, utils.py:502-536)
struct CommitClock {
    bool on; double t0; const char* tag;
    static double now() { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6; }
    explicit CommitClock(const char* tag_) : on(getenv("OWW_COMMIT_TIMING") != nullptr), t0(now()), tag(tag_) {}
    void lap(const char* what) { if (on) { const double t = now(); fprintf(stderr, "[owwhip commit %s] %-28s %8.2f ms\n", tag, what, t - t0); t0 = t; } }
};

// ---- f16-split family: commit-time calibration and self-test against the exact-fp32 kernels -------------------------------------
// The reference's graphs are fp32 (onnxruntime CPU kernels, utils.py:84-93): they have no range to leave.  The f16-split kernels
// carry every activation as an f16 (hi, lo) pair, which is exact to 22 bits only inside the f16 exponent range, so oww_commit
//  (1) runs 32 probe streams (silence ... full-scale noise and square waves) plus the all-ones mel history through a scratch handle
//      of the exact-fp32 family with per-layer dumps and records every layer's largest |activation|,
//  (2) gives every layer the power-of-two scale K = 2^e that puts that maximum at 512..1024 -- a factor 64 below the f16 overflow
//      and 2^13 above the point where the low half goes subnormal -- and folds K, the BatchNorm scale and shift into the packed
//      weights / accumulator start values (fold_cnn; owwhip_hx.h act1),
//  (3) replays the probes through the handle's own f16-split kernels and compares the embeddings (and, with heads loaded, the raw
//      head outputs) with the fp32 run: weights for which the two differ by more than the north-star tolerance are refused with
//      OWW_ERANGE at commit instead of scoring differently later.
// Probes run in batches of CAL_NP streams x CAL_T frames (every handle has at least 32 padded streams): batch 0 is the built-in
// synthetic set, further batches carry the caller's calibration audio (oww_set_calibration: speech), cut into CAL_T-frame segments.
constexpr int CAL_NP = 32, CAL_T = 16, CAL_MAX_BATCHES = 8;
struct HxCalib {
    int nb = 1;                      // batches
    std::vector<int16_t> pcm;        // [nb][CAL_T][CAL_NP][1280]
    DevBuf<int16_t> d_pcm;           // the same on the device: uploaded once, read by the calibration run and by the self-test replay
    std::vector<float> ref_emb;      // [nb][CAL_T][CAL_NP][96]   exact-fp32 embeddings of the probe run
    std::vector<float> ref_raw;      // [nb][CAL_T][CAL_NP][NL]   exact-fp32 raw head outputs
    int NL = 0;
};

void make_probe_pcm(std::vector<int16_t>& pcm, const std::vector<int16_t>& user /*[n_seg][CAL_T * 1280]*/) {
    const size_t seg = (size_t)CAL_T * OWW_CHUNK, n_seg = user.size() / seg;
    const int nb = 1 + (int)((n_seg + CAL_NP - 1) / CAL_NP);
    pcm.assign((size_t)nb * CAL_T * CAL_NP * OWW_CHUNK, 0);
    for (size_t k = 0; k < n_seg; ++k) {
        const size_t b = 1 + k / CAL_NP, i = k % CAL_NP;
        for (int it = 0; it < CAL_T; ++it)
            memcpy(&pcm[((b * CAL_T + it) * CAL_NP + i) * OWW_CHUNK], &user[k * seg + (size_t)it * OWW_CHUNK], OWW_CHUNK * sizeof(int16_t));
    }
    // batch 0 (the synthetic set) is the same for every handle: computed once per process (655,360 Gaussian samples in double)
    static std::once_flag once;
    static std::vector<int16_t> synth;
    std::call_once(once, [] {
        synth.assign((size_t)CAL_T * CAL_NP * OWW_CHUNK, 0);
        uint64_t st = 0x9E3779B97F4A7C15ull;
        auto u01 = [&]() { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return ((st >> 11) + 1) * (1.0 / 9007199254740993.0); };
        const double amps[5] = {30, 300, 3000, 12000, 32767};
        for (int i = 1; i < CAL_NP; ++i) {                 // stream 0: silence
            const double amp = amps[i % 5];
            for (int n = 0; n < CAL_T * OWW_CHUNK; ++n) {
                double v;
                if (i % 3 == 0) v = ((n / (8 << (i % 4))) % 2) ? amp : -amp;                        // square waves, 1 kHz .. 125 Hz
                else v = std::nearbyint(amp * std::sqrt(-2.0 * std::log(u01())) * std::cos(6.283185307179586 * u01()));
                v = std::min(32767.0, std::max(-32768.0, v));
                synth[((size_t)(n / OWW_CHUNK) * CAL_NP + i) * OWW_CHUNK + n % OWW_CHUNK] = (int16_t)v;
            }
        }
    });
    memcpy(pcm.data(), synth.data(), synth.size() * sizeof(int16_t));
}

// one probe step on handle t: mel of the chunk (separate kernel), CNN, frame counters, optionally the heads
int probe_step(oww_ctx* t, const StepArgs& a, const int16_t* d_chunk, bool heads) {
    if (int rc = launch_mel(t, a, d_chunk, CAL_NP, OWW_CHUNK, 8, 1, t->d_mel, nullptr)) return rc;
    if (int rc = run_cnn(t, a, CAL_NP, 256, 0)) return rc;
    if (heads && t->NL > 0)
        if (int rc = run_heads(t, a, CAL_NP, false, nullptr, -1, t->d_raw, 0)) return rc;
    hipLaunchKernelGGL(advance_kernel, dim3((t->Spad + 255) / 256), dim3(256), 0, t->stream, t->d_nfeat, t->Spad, (const uint8_t*)nullptr);
    return 0;
}

// a failure behind queued work: the stream is drained before the caller's local buffers are released at its return
int drained(oww_ctx* h, int rc) { (void)hipStreamSynchronize(h->stream); return rc; }

// the probe run on the scratch exact-fp32 handle t: per-layer maxima into h, reference embeddings and raw scores into cal
int calibrate_run(oww_ctx* h, oww_ctx* t, HxCalib& cal, CommitClock& clk) {
    if (int rc = oww_load_mel(t, h->mel_blob.data(), h->mel_blob.size() * sizeof(float))) return rc;
    if (int rc = oww_load_embedding(t, h->emb_blob.data(), h->emb_blob.size() * sizeof(float))) return rc;
    for (const HeadHost& hh : h->heads) {
        std::vector<float> blob(8 + hh.blob.size());
        const int32_t hdr[8] = {hh.kind, hh.T, hh.hidden, hh.n_out, hh.has_ln, hh.n_blocks - 1, 0, 0};
        memcpy(blob.data(), hdr, sizeof hdr);
        memcpy(blob.data() + 8, hh.blob.data(), hh.blob.size() * sizeof(float));
        if (int rc = oww_add_head(t, blob.data(), blob.size() * sizeof(float)); rc < 0) return rc;
    }
    if (int rc = oww_commit(t)) return rc;
    clk.lap("scratch fp32 handle");
    cal.NL = t->NL;
    int off[21]; off[0] = 0;
    for (int l = 0; l < 20; ++l) off[l + 1] = off[l] + kLayerOut[l][0] * kLayerOut[l][1] * kLayerOut[l][2];
    // probe audio up once, results down once: the run in between is stream-ordered, without a host round trip per probe step
    const size_t n_steps = (size_t)cal.nb * CAL_T, n_emb = n_steps * CAL_NP * 96, n_raw = n_steps * CAL_NP * std::max(t->NL, 1);
    DevBuf<unsigned> d_max; DevBuf<int> d_off; DevBuf<float> d_ref;
    if (d_max.alloc(20) || d_off.alloc(21) || cal.d_pcm.alloc(cal.pcm.size()) || d_ref.alloc(n_emb + n_raw))
        return fail(OWW_ENOMEM, "oww_commit: out of device memory (calibration)");
    if (hipMemsetAsync(d_max, 0, 20 * sizeof(unsigned), t->stream) != hipSuccess ||
        copy_async(d_off, off, sizeof off, hipMemcpyHostToDevice, t->stream) != hipSuccess ||
        copy_async(cal.d_pcm, cal.pcm.data(), cal.pcm.size() * sizeof(int16_t), hipMemcpyHostToDevice, t->stream) != hipSuccess)
        return drained(t, fail(OWW_EHIP, "oww_commit: calibration setup failed"));
    auto absmax = [&]() { hipLaunchKernelGGL(layer_absmax_kernel, dim3(20, CAL_NP), dim3(256), 0, t->stream, t->d_dbg, (size_t)DBG_FLOATS, d_off, d_max); };
    // (a) the all-ones mel history every stream starts from (utils.py:165): the handle sits in that steady state after its commit
    hipLaunchKernelGGL(fill_kernel, dim3(CAL_NP), dim3(256), 0, t->stream, t->d_mel, (size_t)CAL_NP * 256, 1.0f);
    const StepArgs a = step_args(t);             // (every layer dumped: the maxima are read from t's debug buffer)
    if (int rc = run_cnn(t, a, CAL_NP, 256, 0)) return drained(t, rc);
    absmax();
    // (b) the probe audio, batch by batch from the reset state
    cal.ref_emb.assign((size_t)cal.nb * CAL_T * CAL_NP * 96, 0.f);
    cal.ref_raw.assign((size_t)cal.nb * CAL_T * CAL_NP * std::max(t->NL, 1), 0.f);
    for (int bt = 0; bt < cal.nb * CAL_T; ++bt) {
        const int it = bt % CAL_T;
        if (it == 0 && bt > 0) if (int rc = do_reset(t, nullptr, CAL_NP, nullptr)) return drained(t, rc);
        if (getenv("OWW_DEBUG_CALIB")) { const hipError_t e = hipStreamSynchronize(t->stream); fprintf(stderr, "calibrate: probe step %d of %d (%s)\n", bt, cal.nb * CAL_T, hipGetErrorString(e)); }
        if (int rc = probe_step(t, a, cal.d_pcm + (size_t)bt * CAL_NP * OWW_CHUNK, true)) return drained(t, rc);
        absmax();
        if (hipMemcpyAsync(d_ref + (size_t)bt * CAL_NP * 96, t->d_emb, (size_t)CAL_NP * 96 * sizeof(float), hipMemcpyDeviceToDevice, t->stream) != hipSuccess ||
            (t->NL > 0 && hipMemcpyAsync(d_ref + n_emb + (size_t)bt * CAL_NP * t->NL, t->d_raw, (size_t)CAL_NP * t->NL * sizeof(float), hipMemcpyDeviceToDevice, t->stream) != hipSuccess))
            return drained(t, fail(OWW_EHIP, "oww_commit: probe gather failed"));
    }
    unsigned mx[20];
    if (copy_async(cal.ref_emb.data(), d_ref, n_emb * sizeof(float), hipMemcpyDeviceToHost, t->stream) != hipSuccess ||
        (t->NL > 0 && copy_async(cal.ref_raw.data(), d_ref + n_emb, n_raw * sizeof(float), hipMemcpyDeviceToHost, t->stream) != hipSuccess) ||
        copy_async(mx, d_max, sizeof mx, hipMemcpyDeviceToHost, t->stream) != hipSuccess || hipStreamSynchronize(t->stream) != hipSuccess)
        return drained(t, fail(OWW_EHIP, "oww_commit: calibration run failed: %s", hipGetErrorString(hipGetLastError())));
    clk.lap("probe run (exact fp32)");
    for (int l = 0; l < 20; ++l) {
        float m; memcpy(&m, &mx[l], 4);
        if (!std::isfinite(m)) return fail(OWW_EINVAL, "oww_commit: layer %d of the embedding network produces non-finite activations in exact fp32 -- the weights are broken", l);
        h->hx_absmax[l] = m;
    }
    hx_ladder(h->hx_absmax, h->emb_blob, *h);
    return 0;
}

int calibrate_hx(oww_ctx* h, HxCalib& cal) {
    (void)hipGetLastError();                 // (a stale error of the caller's thread is not this function's to report)
    make_probe_pcm(cal.pcm, h->cal_user);
    cal.nb = (int)(cal.pcm.size() / ((size_t)CAL_T * CAL_NP * OWW_CHUNK));
    oww_config c2 = h->cfg;
    c2.n_streams = CAL_NP; c2.max_chunks = 1; c2.use_mfma = 1; c2.debug_layers = 1; c2.stream = nullptr;
    c2.feature_ring = h->TR;
    oww_ctx* t = nullptr;
    if (int rc = oww_create(&c2, &t)) return rc;
    CommitClock clk("calibrate");
    int rc = calibrate_run(h, t, cal, clk);      // (its scratch buffers are gone when it returns)
    const std::string keep = g_err;
    // the scratch handle's whole life -- launches whose status nobody looked at, its frees -- must have left no HIP error behind
    const hipError_t e_run = hipStreamSynchronize(t->stream);
    (void)oww_destroy(t);
    const hipError_t e_last = hipGetLastError();
    if (rc) g_err = keep;
    (void)hipSetDevice(h->cfg.device);
    clk.lap("scratch handle destroyed");
    if (!rc && (e_run != hipSuccess || e_last != hipSuccess))
        rc = fail(OWW_EHIP, "oww_commit: the calibration handle left a HIP error behind (run: %s, last: %s)", hipGetErrorString(e_run), hipGetErrorString(e_last));
    return rc;
}

// replay of the probes on the handle's own (f16-split) kernels; leaves the first CAL_NP streams dirty -- the caller resets all state
int selftest_hx(oww_ctx* h, const HxCalib& cal) {
    const size_t n_steps = (size_t)cal.nb * CAL_T, n_emb = n_steps * CAL_NP * 96, n_raw = n_steps * CAL_NP * std::max(h->NL, 1);
    DevBuf<float> d_out;
    if (!cal.d_pcm) return fail(OWW_ESTATE, "oww_commit: self-test without calibration probes");
    if (d_out.alloc(n_emb + n_raw)) return fail(OWW_ENOMEM, "oww_commit: out of device memory (self-test)");
    std::vector<float> emb(n_emb), raw(n_raw);
    const StepArgs a{};                                  // (no per-layer dumps: the replay runs the kernels the steps run)
    for (int bt = 0; bt < cal.nb * CAL_T; ++bt) {
        if (bt % CAL_T == 0 && bt > 0) if (int rc = do_reset(h, nullptr, CAL_NP, nullptr)) return drained(h, rc);
        if (getenv("OWW_DEBUG_CALIB")) { const hipError_t e = hipStreamSynchronize(h->stream); fprintf(stderr, "self-test: probe step %d of %d (%s)\n", bt, cal.nb * CAL_T, hipGetErrorString(e)); }
        if (int rc = probe_step(h, a, cal.d_pcm + (size_t)bt * CAL_NP * OWW_CHUNK, true)) return drained(h, rc);
        if (hipMemcpyAsync(d_out + (size_t)bt * CAL_NP * 96, h->d_emb, (size_t)CAL_NP * 96 * sizeof(float), hipMemcpyDeviceToDevice, h->stream) != hipSuccess ||
            (h->NL > 0 && hipMemcpyAsync(d_out + n_emb + (size_t)bt * CAL_NP * h->NL, h->d_raw, (size_t)CAL_NP * h->NL * sizeof(float), hipMemcpyDeviceToDevice, h->stream) != hipSuccess))
            return drained(h, fail(OWW_EHIP, "oww_commit: probe gather failed"));
    }
    if (copy_async(emb.data(), d_out, n_emb * sizeof(float), hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
        (h->NL > 0 && copy_async(raw.data(), d_out + n_emb, n_raw * sizeof(float), hipMemcpyDeviceToHost, h->stream) != hipSuccess) ||
        hipStreamSynchronize(h->stream) != hipSuccess) return drained(h, fail(OWW_EHIP, "oww_commit: self-test run failed: %s", hipGetErrorString(hipGetLastError())));
    float err = 0.f, ref = 0.f, serr = 0.f;
    bool finite = true;
    for (size_t i = 0; i < emb.size(); ++i) {
        finite = finite && std::isfinite(emb[i]);
        err = std::max(err, std::fabs(emb[i] - cal.ref_emb[i])); ref = std::max(ref, std::fabs(cal.ref_emb[i]));
    }
    if (h->NL > 0 && cal.NL == h->NL)
        for (size_t i = 0; i < raw.size(); ++i) { finite = finite && std::isfinite(raw[i]); serr = std::max(serr, std::fabs(raw[i] - cal.ref_raw[i])); }
    h->hx_selftest_err = err; h->hx_selftest_ref = ref; h->hx_selftest_score_err = serr;
    if (getenv("OWW_DEBUG_CALIB")) fprintf(stderr, "commit self-test: max |emb - fp32| %.3g on |emb| <= %.3g, max |raw score - fp32| %.3g\n", (double)err, (double)ref, (double)serr);
    const float tol = 1e-3f;                     // the north-star score tolerance
    if (!finite || err > tol * std::max(1.f, ref) || serr > tol || (h->h_range && *(volatile int*)h->h_range)) {
        if (h->h_range) *(volatile int*)h->h_range = 0;
        return fail(OWW_ERANGE, "oww_commit: with these weights the fp16-split kernels (use_mfma = 3) differ from the exact-fp32 kernels by %.3g on "
                    "embeddings of magnitude %.3g and by %.3g on raw scores over the probe set (tolerance %.0e): create the handle with "
                    "use_mfma = 1", (double)err, (double)ref, (double)serr, (double)tol);
    }
    return 0;
}

// ---- head bank helpers (oww_bank_*): their callers have waited for every queued launch of the handle, so the routing table, the bank
//      images and the slot state may change -----------------------------------------------------------------------------------------------
// restart the listed slots (index stream * K + slot): prediction count, ring, raw and final score
int bank_clear(oww_ctx* h, std::vector<int> slots) {
    std::sort(slots.begin(), slots.end());
    slots.erase(std::unique(slots.begin(), slots.end()), slots.end());
    if (slots.empty()) return 0;
    HIPCHK(copy_async(h->d_bank_idx, slots.data(), slots.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(owh::bank_clear_kernel, dim3((unsigned)((slots.size() + 255) / 256)), dim3(256), 0, h->stream, (const int*)h->d_bank_idx,
                       (int)slots.size(), h->d_bank_raw, h->d_bank_scores, h->d_bank_ring, h->d_bank_npred);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));     // (the host list is the copy's source)
    return 0;
}

// Routing table from the subscriptions (owb::route: owwhip_bank_host.h).  One upload per change; the captured step graph is invalidated
// (its launches bake the tile count).
int bank_route(oww_ctx* h) {
    h->bank_rt = owb::route(h->bank_sub.data(), h->S, h->bank_K, h->bank.data(), h->bank_cap, owb::wg_env(), !OWH_BANK_PER_HEAD);
    const owb::Route& r = h->bank_rt;
    HIPCHK(grow(h, h->d_bank_tiles, r.tiles.size()));
    if (!r.tiles.empty()) HIPCHK(copy_sync(h->d_bank_tiles, r.tiles.data(), r.tiles.size() * sizeof(owh::BankTile), hipMemcpyHostToDevice));
    if (!r.entries.empty()) HIPCHK(copy_sync(h->d_bank_entries, r.entries.data(), r.entries.size() * sizeof(int), hipMemcpyHostToDevice));
    if (h->graph_exec) { (void)hipGraphExecDestroy(h->graph_exec); h->graph_exec = nullptr; }     // the launch list changed
    return 0;
}

// ---- per-stream verifier helpers (oww_verifier_*) ------------------------------------------------------------------------------------
// The list stream_verifier_kernel walks, from the assignment tables (owsv::sv_list: owwhip_verifier_host.h).  Callers have quiesced the
// handle's stream; the captured step graph is invalidated (it bakes the list length).
int sv_rebuild(oww_ctx* h) {
    const std::vector<SvEntry> list = owsv::sv_list(h->S, h->NL, h->bank_K, h->vasg_fix, h->vthr_fix, h->vasg_bank, h->vthr_bank, h->vpool_T, h->ver_T,
                                                    h->ver_thr, h->vasg_n);
    if (!list.empty()) HIPCHK(copy_sync(h->d_svlist, list.data(), list.size() * sizeof(SvEntry), hipMemcpyHostToDevice));
    h->sv_n = (int)list.size();
    const unsigned long long zero = 0;
    HIPCHK(copy_sync(h->d_sv_eval, &zero, sizeof zero, hipMemcpyHostToDevice));
    if (h->graph_exec) { (void)hipGraphExecDestroy(h->graph_exec); h->graph_exec = nullptr; }     // the launch list changed
    return 0;
}

// bank slots whose head changed (oww_subscribe, oww_bank_remove) drop their verifier assignment back to the default (none)
int sv_drop_bank(oww_ctx* h, const std::vector<int>& slots) {
    if (h->vpool_cap == 0) return 0;
    bool any = false;
    for (int at : slots)
        if (h->vasg_bank[at] != OWW_VERIFIER_DEFAULT) { h->vasg_bank[at] = OWW_VERIFIER_DEFAULT; --h->vasg_n; any = true; }
    return any ? sv_rebuild(h) : 0;
}

void comm_release(oww_ctx* h) {
    if (h->comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(h->comm);
    h->comm = nullptr; h->comm_rank = 0; h->comm_world = 1;
}

}  // namespace

// Nothing of this handle may still be queued when its buffers go: every stream the handle ever launched on is drained before any member
// is released (hipFree would wait for the whole device as well, but the page-locked words -- h_range, which the f16-split kernels write
// at exit, h_lists, the ingest slots -- and the streams and events themselves are released by calls that promise no such wait).
oww_ctx::~oww_ctx() {
    for (hipStream_t st : {stream.get(), up_stream.get(), down_stream.get()})
        if (st) (void)hipStreamSynchronize(st);
    comm_release(this);
    if (graph_exec) (void)hipGraphExecDestroy(graph_exec);
    if (graph) (void)hipGraphDestroy(graph);
}

namespace {

// ---- oww_commit, phase by phase (the host image phases -- build_nets, pack_* -- are owwhip_pack.h's) ----------------------------------
// upload the image; offsets -> device pointers, the NetDesc tables and the fast groups' HeadHxNets
int bind_weights(oww_ctx* h, const HostBuf& hb, const WeightOff& off) {
    HIPCHK(herr(h->d_w.alloc(hb.data.size())));
    HIPCHK(copy_sync(h->d_w, hb.data.data(), hb.data.size() * sizeof(float), hipMemcpyHostToDevice));
    const float* w = h->d_w;
    h->d_hann = w + off.hann; h->d_mstart = reinterpret_cast<const int*>(w + off.start); h->d_taps = w + off.taps;
    h->d_meloff = reinterpret_cast<const int*>(w + off.meloff); h->d_meldst = reinterpret_cast<const unsigned*>(w + off.meldst);
    if (h->vad) {
        h->d_vad_hann = w + off.vhann; h->d_vad_encw = w + off.vencw; h->d_vad_encb = w + off.vencb;
        h->d_vad_lstmw = w + off.vlw; h->d_vad_lstmb = w + off.vlb; h->d_vad_wd = w + off.vwd;
    }
    for (int l = 0; l < 20; ++l) {
        h->d_conv[l] = w + off.conv[l];
        h->d_scale[l] = l < 19 ? w + off.scale[l] : nullptr;
        h->d_shift[l] = l < 19 ? w + off.shift[l] : nullptr;
    }
    auto make_desc = [&](int ni, int hid_off) {
        const NetHost& n = h->nets[ni];
        const WeightOff::Net& o = off.net[ni];
        NetDesc d{};
        d.hidden = n.hidden; d.n_out = n.n_out; d.has_ln = n.has_ln; d.final_act = n.final_act; d.T = n.T;
        d.head = n.head; d.role = n.role; d.out_col = n.out_col; d.hid_off = hid_off;
        if (n.rnn) { d.rnn = w + o.rnn; return d; }
        d.w1 = w + o.w1; d.b1 = w + o.b1;
        d.ln1g = n.has_ln ? w + o.ln1g : nullptr; d.ln1b = n.has_ln ? w + o.ln1b : nullptr;
        d.n_blocks = n.n_blocks;
        d.blocks = n.n_blocks > 0 ? w + o.blocks : nullptr;
        d.w2 = n.n_blocks > 0 ? w + o.w2 : nullptr; d.b2 = n.n_blocks > 0 ? w + o.b2 : nullptr;
        d.ln2g = n.has_ln && n.n_blocks > 0 ? w + o.ln2g : nullptr; d.ln2b = n.has_ln && n.n_blocks > 0 ? w + o.ln2b : nullptr;
        d.w3 = w + o.w3; d.b3 = w + o.b3;
        d.w2pk = n.hidden == 64 && n.n_blocks == 1 ? w + o.w2pk : nullptr;
        return d;
    };
    if (!h->nets.empty()) {
        std::vector<NetDesc> all;
        for (size_t ni = 0; ni < h->nets.size(); ++ni) all.push_back(make_desc((int)ni, 0));
        HIPCHK(herr(h->d_allnets.alloc(all.size())));
        HIPCHK(copy_sync(h->d_allnets, all.data(), all.size() * sizeof(NetDesc), hipMemcpyHostToDevice));
    }
    for (size_t gi = 0; gi < h->groups.size(); ++gi) {
        FastGroup& g = h->groups[gi];
        const WeightOff::Group& go = off.group[gi];
        std::vector<NetDesc> ds;
        for (int i = 0; i < g.n_nets; ++i) ds.push_back(make_desc(g.nets[i], 64 * i));
        HIPCHK(herr(g.d_nets.alloc(ds.size())));
        HIPCHK(copy_sync(g.d_nets, ds.data(), ds.size() * sizeof(NetDesc), hipMemcpyHostToDevice));
        g.d_w1pk = w + go.w1pk; g.d_b1cat = w + go.b1cat;
        if (!h->hx) continue;
        g.d_w1hx = w + go.w1hx;
        for (int i = 0; i < g.n_nets; ++i)
            g.hx_net.push_back(make_hx_net(h->nets[g.nets[i]], g.ht, go.net[i], w, g.ht == 4 ? w + off.net[g.nets[i]].b3 : nullptr, h->hx_efeat));
    }
    return 0;
}

// sticky range flag of the f16-split kernels: page-locked + device-mapped, so the host reads it without a copy
int alloc_range_flag(oww_ctx* h) {
    void* dp = nullptr;
    HIPCHK(herr(h->h_range.alloc(16, hipHostMallocMapped)));
    h->h_range[0] = 0; h->h_range[1] = -1;
    HIPCHK(hipHostGetDevicePointer(&dp, h->h_range, 0));
    h->d_range = (int*)dp;
    return 0;
}

// every per-stream buffer, zero-filled on the handle's stream
int alloc_state(oww_ctx* h) {
    const size_t SP = h->Spad;
    for (int a = 0; a < N_STATE; ++a) {
        if (int rc = dalloc(h->stream, h->d_state[a], SP * h->state_len[a])) return rc;
        if (int rc = dalloc(h->stream, h->d_tmpl[a], (size_t)h->state_len[a] * (h->rr ? kStateSpgRr[a] : 1))) return rc;
    }
    const int* xlen = h->rr ? kXLenRr : kXLenLds;
    DevBuf<float>* x[4] = {&h->d_xA, &h->d_xB, &h->d_xC, &h->d_xD};
    for (int i = 0; i < 4; ++i) if (int rc = dalloc(h->stream, *x[i], SP * xlen[i])) return rc;
    if (int rc = dalloc(h->stream, h->d_mel, SP * 8 * h->kmax * 32)) return rc;
    if (int rc = dalloc(h->stream, h->d_feat, SP * h->TR * 96)) return rc;
    if (int rc = dalloc(h->stream, h->d_emb, SP * 96)) return rc;
    if (int rc = dalloc(h->stream, h->d_raw, SP * std::max(h->NL, 1))) return rc;
    if (int rc = dalloc(h->stream, h->d_scores, SP * std::max(h->NL, 1))) return rc;
    if (int rc = dalloc(h->stream, h->d_ring, SP * std::max(h->NL, 1) * OWW_SCORE_RING)) return rc;
    if (int rc = dalloc(h->stream, h->d_featinit, (size_t)h->TR * 96)) return rc;
    if (int rc = dalloc(h->stream, h->d_nfeat, SP)) return rc;
    if (int rc = dalloc(h->stream, h->d_npred, SP)) return rc;
    if (int rc = dalloc(h->stream, h->d_vadring, SP * owq::kVadRing)) return rc;
    if (int rc = dalloc(h->stream, h->d_nvad, SP)) return rc;
    if (int rc = dalloc(h->stream, h->d_vadin, SP)) return rc;
    if (h->vad) {
        const size_t G = (SP + 15) / 16;
        if (int rc = dalloc(h->stream, h->d_vadx, G * 4 * 1024)) return rc;
        if (int rc = dalloc(h->stream, h->d_vadhc, G * 4096)) return rc;
        if (int rc = dalloc(h->stream, h->d_vadlast, SP)) return rc;
    }
    if (int rc = dalloc(h->stream, h->d_tail, SP * 480)) return rc;
    if (int rc = dalloc(h->stream, h->d_pcm, (size_t)h->S * OWW_CHUNK * h->kmax)) return rc;
    if (int rc = dalloc(h->stream, h->d_patience, (size_t)std::max(h->NL, 1))) return rc;
    if (int rc = dalloc(h->stream, h->d_threshold, (size_t)std::max(h->NL, 1))) return rc;
    {
        std::vector<float> nanv(std::max(h->NL, 1), NAN);
        HIPCHK(copy_async(h->d_threshold, nanv.data(), nanv.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));   // (behind the buffer's zero fill, same stream)
    }
    if (h->cfg.debug_layers) if (int rc = dalloc(h->stream, h->d_dbg, SP * DBG_FLOATS)) return rc;
    if (const char* e = getenv("OWW_PROF_BLOCK")) { h->prof_block = atoi(e); if (int rc = dalloc(h->stream, h->d_prof, (size_t)4 * 256)) return rc; }
    return 0;
}

// dynamic-LDS limits of the kernels that ask for more than the default
int set_kernel_lds(oww_ctx* h) {
    int rc = 0;
    auto lds = [&rc](auto kernel, int bytes) { if (!rc) rc = set_lds(kernel, bytes); };
    for (const auto& g : h->groups) if (g.ht == 4) lds(heads64_kernel, heads_lds_bytes(g.NH));
    if (!h->rnn_nets.empty()) lds(heads_rnn_kernel<RNN_SPW>, (int)rnn_lds_bytes(RNN_TMAX));
    if (h->vad) lds(owv::vad_front_kernel, owv::V_LDS_BYTES);
    lds(owf::hmelA_kernel<false>, owf::FA_LDS_BYTES); lds(owf::hmelA_kernel<true>, owf::FA_LDS_BYTES);
    lds(owh::hstage_kernel<owh::HB, false, false, owh::RES_B_WG, 1>, owh::RES_B_LDS_BYTES);
    lds(stageA_kernel<true>, CfgA::LDS_BYTES); lds(stageA_kernel<false>, CfgA::LDS_BYTES);
    lds(stage_kernel<CfgB, true, false>, CfgB::LDS_BYTES); lds(stage_kernel<CfgB, false, false>, CfgB::LDS_BYTES);
    lds(stage_kernel<CfgC, true, false>, CfgC::LDS_BYTES); lds(stage_kernel<CfgC, false, false>, CfgC::LDS_BYTES);
    lds(stage_kernel<CfgD, true, false>, CfgD::LDS_BYTES); lds(stage_kernel<CfgD, false, false>, CfgD::LDS_BYTES);
    lds(stage_kernel<CfgE, true, true>, CfgE::LDS_BYTES); lds(stage_kernel<CfgE, false, true>, CfgE::LDS_BYTES);
    return rc;
}

// reset state = what an all-ones mel history leaves behind (utils.py:165 melspectrogram_buffer = ones((76,32))): run the incremental
// CNN on ones rows until the zero start is flushed out, keep the result as the reset template, reset every stream
int derive_reset_state(oww_ctx* h, const HxCalib& cal, CommitClock& clk) {
    const size_t SP = h->Spad;
    const int warm = std::min<int>(32, (int)SP);
    hipLaunchKernelGGL(fill_kernel, dim3((warm * 256 + 255) / 256), dim3(256), 0, h->stream, h->d_mel, (size_t)warm * 256, 1.0f);
    const StepArgs args{};                             // (no per-layer dumps)
    for (int it = 0; it < 12; ++it)
        if (int rc = run_cnn(h, args, warm, 256, 0)) return rc;
    for (int a = 0; a < N_STATE; ++a)
        HIPCHK(copy_async(h->d_tmpl[a], h->d_state[a], (size_t)h->state_len[a] * (h->rr ? kStateSpgRr[a] : 1) * sizeof(float),
                              hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipMemsetAsync(h->d_mel, 0, SP * 8 * h->kmax * 32 * sizeof(float), h->stream));
    HIPCHK(hipMemsetAsync(h->d_emb, 0, SP * 96 * sizeof(float), h->stream));
    if (int rc = do_reset(h, nullptr, (int)SP, nullptr)) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    clk.lap("warm-up + reset");
    // the warm-up already drove the network with an all-ones mel history: weights that overflow the f16 range there are refused now
    if (int rc = range_check(h, "oww_commit")) return rc;
    // f16-split family: replay the calibration probes and hold the result to the exact-fp32 run (refuses weights the split loses)
    if (h->hx && !getenv("OWW_NO_COMMIT_SELFTEST")) {
        if (int rc = selftest_hx(h, cal)) return rc;
        HIPCHK(hipMemsetAsync(h->d_mel, 0, SP * 8 * h->kmax * 32 * sizeof(float), h->stream));
        HIPCHK(hipMemsetAsync(h->d_emb, 0, SP * 96 * sizeof(float), h->stream));
        HIPCHK(hipMemsetAsync(h->d_raw, 0, SP * std::max(h->NL, 1) * sizeof(float), h->stream));
        if (int rc = do_reset(h, nullptr, (int)SP, nullptr)) return rc;
        HIPCHK(hipStreamSynchronize(h->stream));
        clk.lap("self-test replay + reset");
    }
    return 0;
}

// head bank (oww_bank_configure): subscription table, per-slot outputs, the head table; no head yet
int alloc_bank(oww_ctx* h) {
    const size_t SK = (size_t)h->S * h->bank_K;
    if (int rc = dalloc(h->stream, h->d_bank_sub, SK, false)) return rc;
    if (int rc = dalloc(h->stream, h->d_bank_idx, SK)) return rc;
    if (int rc = dalloc(h->stream, h->d_bank_raw, SK)) return rc;
    if (int rc = dalloc(h->stream, h->d_bank_scores, SK)) return rc;
    if (int rc = dalloc(h->stream, h->d_bank_ring, SK * OWW_SCORE_RING)) return rc;
    if (int rc = dalloc(h->stream, h->d_bank_npred, SK)) return rc;
    if (int rc = dalloc(h->stream, h->d_bank_entries, SK)) return rc;
    if (int rc = dalloc(h->stream, h->d_bank_heads, (size_t)h->bank_cap)) return rc;
    if (int rc = dalloc(h->stream, h->d_bank_pat, (size_t)h->bank_cap)) return rc;
    if (int rc = dalloc(h->stream, h->d_bank_thr, (size_t)h->bank_cap, false)) return rc;
    h->bank.clear(); h->bank.resize(h->bank_cap);
    h->bank_sub.assign(SK, -1);
    std::vector<float> nanv(h->bank_cap, NAN);
    HIPCHK(copy_async(h->d_bank_sub, h->bank_sub.data(), SK * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(copy_async(h->d_bank_thr, nanv.data(), nanv.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

// per-stream verifiers (oww_verifier_configure): the pool, the assignment tables (every pair at the default) and the pair list
int alloc_verifiers(oww_ctx* h) {
    h->vpool_stride = h->TR * OWW_EMB_DIM;
    if (int rc = dalloc(h->stream, h->d_vpool_w, (size_t)h->vpool_cap * h->vpool_stride)) return rc;
    if (int rc = dalloc(h->stream, h->d_vpool_b, (size_t)h->vpool_cap)) return rc;
    if (int rc = dalloc(h->stream, h->d_svlist, (size_t)h->S * (h->NL + h->bank_K), false)) return rc;
    if (int rc = dalloc(h->stream, h->d_sv_eval, 1)) return rc;
    h->vpool_T.assign(h->vpool_cap, 0);
    h->vasg_fix.assign((size_t)h->S * h->NL, OWW_VERIFIER_DEFAULT);
    h->vthr_fix.assign((size_t)h->S * h->NL, 0.f);
    h->vasg_bank.assign((size_t)h->S * h->bank_K, OWW_VERIFIER_DEFAULT);
    h->vthr_bank.assign((size_t)h->S * h->bank_K, 0.f);
    h->vasg_n = 0; h->sv_n = 0;
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

// ---- stream state records (oww_state_info / oww_state_export / oww_state_import / oww_move_streams; kernels in owwhip_state.h) ---------

// Record layout and fingerprint of this handle (ows::layout, ows::fingerprint: owwhip_state_host.h), and the device copy of the flat
// section table.  Built by the first call that needs it: a handle that never exports, imports or moves a stream allocates nothing here.
int state_layout(oww_ctx* h) {
    if (h->st_ready) return 0;
    h->st_flat.clear(); h->st_group.clear();
    auto flat = [&](void* live, size_t stride, size_t len) { h->st_flat.push_back(ows::FlatSection{static_cast<uint32_t*>(live), (uint32_t)stride, (uint32_t)len, 0, 0}); };
    const bool il = h->hx && owh::kInterleave;
    const size_t NL = (size_t)h->NL, K = (size_t)h->bank_K;
    for (int a = 0; a < N_STATE; ++a)
        if (!h->rr || kStateSpgRr[a] == 1) flat(h->d_state[a], h->state_len[a], h->state_len[a]);
    flat(h->d_tail, 240, 240);                                            // 480 int16 samples
    flat(h->d_feat, (size_t)h->TR * OWW_EMB_DIM, (size_t)h->TR * OWW_EMB_DIM);
    flat(h->d_ring, NL * OWW_SCORE_RING, NL * OWW_SCORE_RING);
    flat(h->d_raw, NL, NL); flat(h->d_scores, NL, NL);
    flat(h->d_nfeat, 1, 1); flat(h->d_npred, 1, 1);
    flat(h->d_vadring, owq::kVadRing, owq::kVadRing); flat(h->d_nvad, 1, 1);
    if (h->vad) flat(h->d_vadlast, 1, 1);
    if (K) { flat(h->d_bank_raw, K, K); flat(h->d_bank_scores, K, K); flat(h->d_bank_npred, K, K); flat(h->d_bank_ring, K * OWW_SCORE_RING, K * OWW_SCORE_RING); }
    const oww_ctx::Ingest& ing = h->ing;
    if (ing.ready && ing.tab.Hpad_max) flat(ing.d_hist, (size_t)ing.tab.Hpad_max / 2, (size_t)ing.tab.Hpad_max / 2);   // oww_ingest history (int16 pairs)
    if (ing.ready && ing.mixed) flat(ing.d_cls, 1, 1);                     // ... and the stream's class: one word in a 16-byte piece of its own
    if (audio_on(h)) {                                                     // the ring as it lies, then the counter in a 16-byte piece of its own
        flat(h->d_aring, owa::ring_words(h->aud_ring), owa::ring_words(h->aud_ring));
        flat(h->d_acount, owa::kCounterWords, owa::kCounterWords);
    }
    for (int a = 0; a < N_STATE; ++a)
        if (h->rr && kStateSpgRr[a] > 1)
            h->st_group.push_back(ows::GroupSection{h->d_state[a], kStateSpgRr[a], il ? 16 / kStateSpgRr[a] : kStateFposRr[a], il, (uint32_t)(h->state_len[a] * kStateSpgRr[a]), 0});
    if (h->vad) h->st_group.push_back(ows::GroupSection{h->d_vadhc, 16, 1, true, 4096, 0});      // (h, c): [4 arrays][16 registers][4 j][16 streams]
    ows::Layout L;
    if (int rc = ows::layout(h->st_flat, h->st_group, L)) return rc;
    h->st_flat_quads = L.flat_quads; h->st_record_words = L.record_words;
    for (int lv = 0; lv < 4; ++lv) {
        h->st_levels[lv] = false;
        for (const auto& g : h->st_group) h->st_levels[lv] = h->st_levels[lv] || g.spg == ows::kStateLevels[lv];
    }
    std::vector<ows::HeadPrint> heads;
    for (const auto& hh : h->heads) heads.push_back(ows::HeadPrint{{hh.kind, hh.T, hh.hidden, hh.n_out, hh.has_ln, hh.n_blocks}, {hh.blob.data(), hh.blob.size() * sizeof(float)}});
    const uint64_t fp = ows::fingerprint(h->cfg.use_mfma, il, h->state_len, N_STATE, h->TR, h->NL, h->bank_K, h->vad, h->hx ? h->hx_e : nullptr, h->hx_efeat,
                                         {h->mel_blob.data(), h->mel_blob.size() * sizeof(float)}, {h->emb_blob.data(), h->emb_blob.size() * sizeof(float)}, heads,
                                         {h->vad_blob.data(), h->vad_blob.size() * sizeof(float)});
    h->st_fp = owa::fingerprint(owi::fingerprint(fp, ing.ready, ing.mixed, ing.tab), h->aud_ring);
    if (!h->d_st_flat) HIPCHK(herr(h->d_st_flat.alloc(h->st_flat.size())));
    HIPCHK(copy_sync(h->d_st_flat, h->st_flat.data(), h->st_flat.size() * sizeof(ows::FlatSection), hipMemcpyHostToDevice));
    h->st_ready = true;
    return 0;
}

int state_lists_upload(oww_ctx* h, const std::vector<int>& buf) {
    if (grow(h, h->d_st_items, buf.size()) != hipSuccess) return fail(OWW_ENOMEM, "out of device memory for %zu stream list bytes", buf.size() * sizeof(int));
    HIPCHK(copy_async(h->d_st_items, buf.data(), buf.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    return 0;
}

int state_stage(oww_ctx* h, size_t n) {
    const size_t need = n * (size_t)h->st_record_words;
    if (grow(h, h->d_st_stage, need) != hipSuccess) return fail(OWW_ENOMEM, "out of device memory for %zu bytes of stream state records", need * 4);
    return 0;
}

// gather (SCATTER = false: live -> rec) or scatter (rec -> live) of one uploaded list, on the handle's stream
template <bool SCATTER>
int state_xfer(oww_ctx* h, const ows::StateList& L, uint32_t* rec) {
    if (L.n == 0) return 0;
    ows::FlatParams fp{};
    fp.ids = h->d_st_items + L.ids_at; fp.sec = h->d_st_flat; fp.n_sec = (int)h->st_flat.size(); fp.flat_quads = h->st_flat_quads;
    fp.rec = rec; fp.record_words = h->st_record_words; fp.record_bytes = h->st_record_words * 4;
    fp.fp_lo = (uint32_t)h->st_fp; fp.fp_hi = (uint32_t)(h->st_fp >> 32);
    hipLaunchKernelGGL(ows::state_flat_kernel<SCATTER>, dim3(L.n, (h->st_flat_quads + 255) / 256), dim3(256), 0, h->stream, fp);
    HIPCHK(hipGetLastError());
    for (const auto& g : h->st_group) {
        int lv = 0;
        while (ows::kStateLevels[lv] != g.spg) ++lv;
        if (L.n_groups[lv] == 0) continue;
        ows::GroupParams gp{};
        const int R = g.ppr >= 4 ? 1 : 4 / g.ppr;
        gp.live = reinterpret_cast<uint32_t*>(g.live); gp.block_words = g.block_words; gp.items = h->d_st_items + L.items_at[lv];
        gp.n_chunks = (int)(g.block_words / (16 * R)); gp.rec = rec; gp.record_words = h->st_record_words; gp.off = g.off;
        const dim3 grid(L.n_groups[lv], (gp.n_chunks + 63) / 64);
#define OWS_GO(SPG, PPR, IL) hipLaunchKernelGGL((ows::state_group_kernel<SPG, PPR, IL, SCATTER>), grid, dim3(64), 0, h->stream, gp)
        if (g.il) {
            if (g.spg == 2) OWS_GO(2, 8, true); else if (g.spg == 4) OWS_GO(4, 4, true); else if (g.spg == 8) OWS_GO(8, 2, true); else OWS_GO(16, 1, true);
        } else {
            if (g.spg == 2 && g.ppr == 8) OWS_GO(2, 8, false); else if (g.spg == 4 && g.ppr == 4) OWS_GO(4, 4, false);
            else if (g.spg == 8 && g.ppr == 2) OWS_GO(8, 2, false); else if (g.spg == 8 && g.ppr == 1) OWS_GO(8, 1, false);
            else return fail(OWW_ESTATE, "state records: no kernel for %d streams x %d positions per block", g.spg, g.ppr);
        }
#undef OWS_GO
        HIPCHK(hipGetLastError());
    }
    return 0;
}

// the stream ids of a reset, into d_ids on the handle's stream
int upload_ids(oww_ctx* h, const int32_t* ids, int n) {
    HIPCHK(grow(h, h->d_ids, (size_t)n));
    HIPCHK(copy_async(h->d_ids, ids, (size_t)n * sizeof(int), hipMemcpyHostToDevice, h->stream));
    return 0;
}

// The end of every step entry point: the scores out and, with sync -- somebody's host buffer must be free / filled on return -- the
// wait and the range check behind it.
int deliver_scores(oww_ctx* h, float* scores, int scores_on_device, bool sync, const char* fn) {
    const size_t nb = (size_t)h->S * h->NL * sizeof(float);
    if (scores && nb) HIPCHK(copy_async(scores, h->d_scores, nb, scores_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream));
    if (!sync) return OWW_OK;
    HIPCHK(hipStreamSynchronize(h->stream));
    return range_check(h, fn);
}

// oww_step_masked / oww_submit_masked: the handle's own mask buffer (the kernels index it up to the padded stream count: pad streams 0)
int ensure_mask(oww_ctx* h) {
    if (h->d_on) return 0;
    HIPCHK(herr(h->d_on.alloc(h->Spad)));
    HIPCHK(hipMemsetAsync(h->d_on, 0, h->Spad, h->stream));
    return 0;
}

}  // namespace

// =====================================================================================================
// ---- dense scoring (oww_score_*; owwhip_dense.h, owwhip_dense_host.h) ------------------------------------------------------------------
namespace {

int dense_t_max(const oww_ctx* h) {
    int t = 0;
    for (const HeadHost& hh : h->heads) t = std::max(t, hh.T);
    return t;
}

// One launch of a sliding kernel, fixed heads or bank: k4 / k3 / k2 are its instantiations for a ring of 4, 3 and 2 slots
// (owd::geometry; its staged rows are the dynamic LDS).  (The attribute call stays in front of the timed window: with an idle device the
// start event is stamped at once, and host time between it and the launch would be booked as kernel time.)
template <class P>
int launch_dense(oww_ctx* h, const owd::Geometry& geo, dim3 grid, const P& q, void (*k4)(P), void (*k3)(P), void (*k2)(P)) {
    void (*const k)(P) = geo.slots >= 4 ? k4 : geo.slots == 3 ? k3 : k2;
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)geo.staged));
    Timed t(h, 6);
    hipLaunchKernelGGL(k, grid, dim3(64 * geo.waves), (int)geo.staged, h->stream, q);
    return 0;
}
template <int NN, int WG>
int launch_dense_nn(oww_ctx* h, const owd::Geometry& geo, dim3 grid, const owh::DenseParams& q) {
    if (q.mask) return launch_dense(h, geo, grid, q, owh::heads_dense_kernel<NN, 4, WG, true>, owh::heads_dense_kernel<NN, 3, WG, true>, owh::heads_dense_kernel<NN, 2, WG, true>);
    return launch_dense(h, geo, grid, q, owh::heads_dense_kernel<NN, 4, WG>, owh::heads_dense_kernel<NN, 3, WG>, owh::heads_dense_kernel<NN, 2, WG>);
}
template <int WG>
int launch_dense_bank(oww_ctx* h, const owd::Geometry& geo, dim3 grid, const owh::DenseBankParams& q) {
    if (q.mask) return launch_dense(h, geo, grid, q, owh::heads_dense_bank_kernel<4, WG, true>, owh::heads_dense_bank_kernel<3, WG, true>, owh::heads_dense_bank_kernel<2, WG, true>);
    return launch_dense(h, geo, grid, q, owh::heads_dense_bank_kernel<4, WG>, owh::heads_dense_bank_kernel<3, WG>, owh::heads_dense_bank_kernel<2, WG>);
}

// Where the hit-list entries send a call's scores instead of the matrix: the mask [n_cols][col_stride] (owdh::col_stride; words per
// sequence wps), against thresholds d_thr on the device and thr on the host.  The fallback forms OR their bits in (dense_hits_slab_kernel).
struct MaskSink {
    unsigned* mask; int64_t col_stride, wps;
    const float* d_thr; const float* thr;
};
void launch_hits_slab(oww_ctx* h, const MaskSink& ms, const float* scores, int stride, int off, int col, int64_t nw, int64_t first, int64_t n) {
    owh::HitSlabParams sp{};
    sp.scores = scores; sp.stride = stride; sp.off = off; sp.n_win = nw; sp.first = first; sp.n = n; sp.thr = ms.thr[col];
    sp.mask = ms.mask + (size_t)col * ms.col_stride; sp.wps = ms.wps;
    Timed t(h, 7);
    hipLaunchKernelGGL(owh::dense_hits_slab_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, sp);
}

// the A/B aids of both dense paths: OWW_DENSE_PATH=ext = every head down the gather fallback, OWW_DENSE_SLAB_MB = the slab budget
struct DenseEnv { bool slide; int64_t budget; };
DenseEnv dense_env() {
    const char* path = getenv("OWW_DENSE_PATH");
    const char* mb = getenv("OWW_DENSE_SLAB_MB");
    return DenseEnv{!(path && !strcmp(path, "ext")), mb ? std::max<int64_t>(1, atoll(mb)) << 20 : owd::kSlabBytes};
}

// The gather fallback of one call: the windows of d_feats [B][n_rows][96] materialised into a bounded slab, slab after slab.  want(T)
// for every head that takes it sizes the slab, each(h, T, f) gathers a head's windows slab by slab and hands f(first, n) -- windows
// [first, first + n) of the flattened [B][nw] list are in d_slab -- to the caller's head launches; it stops at f's first error.
struct SlabWalk {
    const float* d_feats; int B, n_rows, t_max; int64_t nw, budget;
    int64_t bytes = 0, windows = 0;             // of the largest slab wanted (0: nobody takes the fallback)
    DevBuf<float> d_slab;
    void want(int T) { const owd::Slab sl = owd::slab((int64_t)B * nw, T, budget); bytes = std::max(bytes, sl.bytes); windows = std::max(windows, sl.windows); }
    template <class F>
    int each(oww_ctx* h, int T, F&& f) {
        const owd::Slab sl = owd::slab((int64_t)B * nw, T, budget);
        for (int64_t s = 0; s < sl.n_slabs; ++s) {
            const int64_t first = s * sl.windows, n = std::min<int64_t>(sl.windows, (int64_t)B * nw - first);
            owh::GatherParams gp{};
            gp.feats = d_feats + (size_t)owd::row_offset(t_max, T) * 96; gp.seq_stride = (long long)n_rows * 96;
            gp.n_win = nw; gp.first = first; gp.n = n; gp.T = T; gp.slab = d_slab;
            {
                Timed t(h, 7);
                const int64_t pieces = n * T * 24;
                hipLaunchKernelGGL(owh::dense_gather_kernel, dim3((unsigned)std::min<int64_t>((pieces + 255) / 256, 256 * 16)), dim3(256), 0, h->stream, gp);
            }
            if (int rc = f(first, n)) return rc;
        }
        return 0;
    }
};

// every window of d_feats [B][n_rows][96] through every fixed head -> d_out [B][n_win][NL]; both on the device.  Narrow fp16-split
// groups take the sliding-window kernel, one launch per pass of one or two nets (owd::split_passes, owd::geometry); every other head
// -- wide and generic nets, recurrent heads, the fp32 and LDS-tiled families, a T whose rows do not fit the LDS -- has its windows
// gathered into a bounded slab and scored by run_heads as external features, slab after slab.  OWW_DENSE_PATH=ext (A/B aid) sends
// every head down the second path.
int score_device(oww_ctx* h, const char* fn, const float* d_feats, int B, int n_rows, float* d_out, const MaskSink* ms = nullptr) {
    const int t_max = dense_t_max(h);
    const int64_t nw = owd::n_win(n_rows, t_max);
    const DenseEnv env = dense_env();
    const bool slide = h->hx && h->mfma && env.slide;
    // d_out is not cleared (it may be gigabytes): every fixed head is scored below, by a sliding pass or by the fallback, and the
    // heads' n_out columns are exactly the NL columns of a row (build_nets lays them side by side), so every entry is written
    std::vector<char> covered(h->heads.size(), 0);
    if (slide) {
        for (const FastGroup& g : h->groups) {
            if (g.ht != 4 || g.n_nets > 4 || !owd::geometry(owd::kMaxPassNets, g.T).slots) continue;      // (two nets fit: so does one)
            int role[4], head[4], pass[4][2];
            for (int i = 0; i < g.n_nets; ++i) { role[i] = g.hx_net[i].role; head[i] = g.hx_net[i].head; }
            const int n_pass = owd::split_passes(role, head, g.n_nets, pass);
            const int off = (int)owd::row_offset(t_max, g.T);
            for (int k = 0; k < n_pass; ++k) {
                const int n0 = pass[k][0], nn = pass[k][1];
                const owd::Geometry geo = owd::geometry(nn, g.T);
                owh::DenseParams q{};
                q.feats = d_feats + (size_t)off * 96; q.seq_stride = (long long)n_rows * 96; q.n_rows = n_rows - off;
                q.n_win = (int)nw; q.tiles = (int)owd::tiles_per_seq(nw, geo.waves); q.T = g.T;
                q.w1hx = g.d_w1hx + (size_t)n0 * 4 * 2 * 256; q.chunk_stride = g.n_nets * 4 * 2 * 256;
                for (int i = 0; i < nn; ++i) q.net[i] = g.hx_net[n0 + i];
                q.out = d_out; q.NL = h->NL; q.range_flag = h->d_range; q.fscale = std::ldexp(1.0f, h->hx_efeat);
                if (ms) { q.mask = ms->mask; q.mask_col_stride = ms->col_stride; q.mask_wps = (int)ms->wps; q.thr = ms->d_thr; }
                const dim3 grid((unsigned)((int64_t)B * q.tiles));
                int rc = 0;
                if (geo.waves == owd::kWavesBig) rc = nn == 1 ? launch_dense_nn<1, owd::kWavesBig>(h, geo, grid, q) : launch_dense_nn<2, owd::kWavesBig>(h, geo, grid, q);
                else rc = nn == 1 ? launch_dense_nn<1, owd::kWavesSmall>(h, geo, grid, q) : launch_dense_nn<2, owd::kWavesSmall>(h, geo, grid, q);
                if (rc) return rc;
            }
            for (int ni : g.nets) covered[h->nets[ni].head] = 1;
        }
        HIPCHK(hipGetLastError());
    }
    // what is left, one launch unit at a time: a fast group the kernel above did not take is ONE run_heads launch for all its heads
    // (run_heads launches the whole group of the head it is asked for), a generic or recurrent head is a launch of its own
    SlabWalk sw{d_feats, B, n_rows, t_max, nw, env.budget};
    for (size_t hi = 0; hi < h->heads.size(); ++hi)
        if (!covered[hi]) sw.want(h->heads[hi].T);
    if (!sw.bytes) return 0;
    if (sw.d_slab.alloc((size_t)sw.bytes / sizeof(float))) return fail(OWW_ENOMEM, "%s: out of device memory (%lld bytes of window slab)", fn, (long long)sw.bytes);
    DevBuf<float> d_scr;            // hit lists: a slab's scores [windows][NL] instead of the matrix's rows
    if (ms && d_scr.alloc((size_t)sw.windows * h->NL))
        return fail(OWW_ENOMEM, "%s: out of device memory (%lld bytes of slab scores)", fn, (long long)sw.windows * h->NL * 4);
    int rc = 0;
    for (size_t hi = 0; hi < h->heads.size() && !rc; ++hi) {
        if (covered[hi]) continue;
        std::vector<int> launched{(int)hi};         // the heads one run_heads launch scores: hi and, on the MFMA families, its group
        if (ms && h->mfma)
            for (const FastGroup& g : h->groups) {
                bool has = false;
                for (int ni : g.nets) has |= h->nets[ni].head == (int)hi;
                if (has) for (int ni : g.nets) if (std::find(launched.begin(), launched.end(), h->nets[ni].head) == launched.end()) launched.push_back(h->nets[ni].head);
            }
        if (ms)     // a fallback column's bits are ORed in, so its words start at 0 (a sliding pass overwrites every word of its own)
            for (int lh : launched)
                if (hipMemsetAsync(ms->mask + (size_t)h->heads[lh].out_col * ms->col_stride, 0, (size_t)h->heads[lh].n_out * ms->col_stride * 4, h->stream) != hipSuccess)
                    return drained(h, fail(OWW_EHIP, "%s: clearing the hit mask failed", fn));
        rc = sw.each(h, h->heads[hi].T, [&](int64_t first, int64_t n) {
            if (!ms) return run_heads(h, step_args(h), (int)n, false, sw.d_slab, (int)hi, d_out + (size_t)first * h->NL, 0);
            if (int r = run_heads(h, step_args(h), (int)n, false, sw.d_slab, (int)hi, d_scr, 0)) return r;
            for (int lh : launched)
                for (int o = 0; o < h->heads[lh].n_out; ++o)
                    launch_hits_slab(h, *ms, d_scr, h->NL, h->heads[lh].out_col + o, h->heads[lh].out_col + o, nw, first, n);
            return 0;
        });
        covered[hi] = 1;
        if (h->mfma)
            for (const FastGroup& g : h->groups) {
                bool has = false;
                for (int ni : g.nets) has |= h->nets[ni].head == (int)hi;
                if (has) for (int ni : g.nets) covered[h->nets[ni].head] = 1;      // (scored by the launches above, same T)
            }
    }
    return drained(h, rc);          // (the slab goes with this scope)
}

// ---- dense scoring over the head bank (oww_bank_score_*; owwhip_dense.h: heads_dense_bank_kernel, owwhip_dense_bank_host.h) ----------
// T of every live bank head by id (0 = empty slot): what owd::bank_ids_check reads
std::vector<int> bank_live_T(const oww_ctx* h) {
    std::vector<int> t(h->bank.size(), 0);
    for (size_t i = 0; i < h->bank.size(); ++i) if (h->bank[i].live) t[i] = h->bank[i].T;
    return t;
}

// n windows of a slab [n][T][96] through ONE bank head by heads_bank_kernel in its ext mode (the launch of oww_bank_add's self-test) ->
// d_sc[n]: what bank_score_device's fallback and the hit lists' re-score (BankRescorer) both run.  prepare() sizes the score, entry and
// tile lists for the largest slab; the tile list is rebuilt where a slab's window count differs from the last one's.
struct BankExtScorer {
    oww_ctx* h; const char* fn;
    DevBuf<float> d_sc; DevBuf<int> d_ent; DevBuf<owh::BankTile> d_til;
    std::vector<int> ent; std::vector<owh::BankTile> til;
    int64_t til_n = -1;                         // the window count d_til describes
    static int64_t bytes(int64_t max_windows) { return max_windows * 8 + (max_windows + 127) / 128 * 16; }
    int prepare(int64_t max_windows) {
        if (d_sc.alloc((size_t)max_windows) || d_ent.alloc((size_t)max_windows) || d_til.alloc((size_t)((max_windows + 127) / 128)))
            return fail(OWW_ENOMEM, "%s: out of device memory (%lld bytes of slab scores and lists)", fn, (long long)bytes(max_windows));
        ent.resize((size_t)max_windows);
        for (int64_t k = 0; k < max_windows; ++k) ent[(size_t)k] = (int)k;
        if (copy_async(d_ent, ent.data(), ent.size() * sizeof(int), hipMemcpyHostToDevice, h->stream) != hipSuccess) return fail(OWW_EHIP, "%s: H2D failed", fn);
        return 0;
    }
    int score(int id, const float* d_slab, int64_t n) {
        if (n != til_n) {                       // (the launches that read the old list, and the gather just enqueued, end first)
            if (hipStreamSynchronize(h->stream) != hipSuccess) return fail(OWW_EHIP, "%s: device error: %s", fn, hipGetErrorString(hipGetLastError()));
            til.clear();
            for (int64_t o0 = 0; o0 < n; o0 += 128) til.push_back(owh::BankTile{0, (int)o0, (int)std::min<int64_t>(128, n - o0), 0});
            if (copy_sync(d_til, til.data(), til.size() * sizeof(owh::BankTile), hipMemcpyHostToDevice) != hipSuccess) return fail(OWW_EHIP, "%s: H2D failed", fn);
            til_n = n;
        }
        const oww_ctx::BankHead& bh = h->bank[id];
        owh::BankParams bp{};
        bp.feat = d_slab; bp.ext = 1; bp.TR = bh.T; bp.tiles = d_til; bp.entries = d_ent; bp.heads = h->d_bank_heads + id; bp.K = 1;
        bp.raw = d_sc; bp.range_flag = h->d_range; bp.fscale = std::ldexp(1.0f, h->hx_efeat);
        Timed t(h, 6);
        const dim3 grid((unsigned)til.size());
        if (bh.ht == 4) hipLaunchKernelGGL((owh::heads_bank_kernel<4, 4>), grid, dim3(256), 0, h->stream, bp);
        else hipLaunchKernelGGL((owh::heads_bank_kernel<4, 8>), grid, dim3(256), 0, h->stream, bp);
        return 0;
    }
};

// every window of d_feats [B][n_rows][96] through the listed bank heads (checked: live; t_max their largest T) -> d_out [B][n_win][n_ids]
// or, d_out == nullptr, into the statistics d_count / d_key [B][n_ids] (cleared by the caller) against d_thr / thr [n_ids].  The narrow
// heads (ht 4) run as ONE launch of heads_dense_bank_kernel on the slice plan; wide heads, whatever the plan refuses and, with
// OWW_DENSE_PATH=ext, everything take the fallback head by head: windows gathered into the bounded slab, heads_bank_kernel in its ext
// mode (the launch of oww_bank_add's self-test), dense_bank_slab_kernel from the slab's scores into the column or the statistics.
int bank_score_device(oww_ctx* h, const char* fn, const float* d_feats, int B, int n_rows, const int32_t* ids, int n_ids, int t_max, float* d_out,
                      const float* d_thr, const float* thr, int* d_count, unsigned long long* d_key, const MaskSink* ms = nullptr) {
    const int64_t nw = owd::n_win(n_rows, t_max);
    const DenseEnv env = dense_env();
    const float fscale = std::ldexp(1.0f, h->hx_efeat);
    std::vector<owh::DenseBankItem> items;
    int t_s = 0;
    for (int i = 0; i < n_ids; ++i)
        if (env.slide && h->bank[ids[i]].ht == 4) { items.push_back(owh::DenseBankItem{ids[i], i}); t_s = std::max(t_s, h->bank[ids[i]].T); }
    const owd::BankPlan plan = items.empty() ? owd::BankPlan{} : owd::bank_plan((int64_t)items.size(), B, nw, t_s, owd::bank_hpw_env());
    if (!plan.hpw) items.clear();
    std::vector<char> covered((size_t)n_ids, 0);
    DevBuf<owh::DenseBankItem> d_items;
    if (!items.empty()) {
        if (d_items.alloc(items.size())) return fail(OWW_ENOMEM, "%s: out of device memory (%zu bytes of head list)", fn, items.size() * sizeof(owh::DenseBankItem));
        if (copy_async(d_items, items.data(), items.size() * sizeof(owh::DenseBankItem), hipMemcpyHostToDevice, h->stream) != hipSuccess)
            return fail(OWW_EHIP, "%s: H2D failed", fn);
        const int off = (int)owd::row_offset(t_max, t_s);
        owh::DenseBankParams q{};
        q.feats = d_feats + (size_t)off * 96; q.seq_stride = (long long)n_rows * 96; q.n_rows = n_rows - off;
        q.n_win = (int)nw; q.seq_tiles = (int)plan.seq_tiles; q.tiles = (int)plan.tiles; q.t_s = t_s;
        q.heads = h->d_bank_heads; q.items = d_items; q.n_items = (int)items.size(); q.hpw = plan.hpw;
        q.out = d_out; q.n_ids = n_ids; q.thr = d_thr; q.count = d_count; q.key = d_key; q.range_flag = h->d_range; q.fscale = fscale;
        if (ms) { q.mask = ms->mask; q.mask_col_stride = ms->col_stride; q.mask_wps = (int)ms->wps; q.thr = ms->d_thr; }
        const dim3 grid((unsigned)plan.grid);
        if (int rc = plan.geo.waves == owd::kWavesBig ? launch_dense_bank<owd::kWavesBig>(h, plan.geo, grid, q)
                                                      : launch_dense_bank<owd::kWavesSmall>(h, plan.geo, grid, q)) return drained(h, rc);
        HIPCHK(hipGetLastError());
        for (const owh::DenseBankItem& it : items) covered[it.col] = 1;
    }
    // ---- the fallback, one head at a time
    SlabWalk sw{d_feats, B, n_rows, t_max, nw, env.budget};
    for (int i = 0; i < n_ids; ++i)
        if (!covered[i]) sw.want(h->bank[ids[i]].T);
    if (!sw.bytes) return drained(h, 0);        // (the head list is the copy's source)
    if (sw.d_slab.alloc((size_t)sw.bytes / sizeof(float)))
        return drained(h, fail(OWW_ENOMEM, "%s: out of device memory (%lld bytes of window slab)", fn, (long long)(sw.bytes + BankExtScorer::bytes(sw.windows))));
    BankExtScorer ext{h, fn};
    if (int rc = ext.prepare(sw.windows)) return drained(h, rc);
    for (int i = 0; i < n_ids; ++i) {
        if (covered[i]) continue;
        // hit lists: a fallback column's bits are ORed in, so its words start at 0 (the sliding launch overwrites every word of its own)
        if (ms && hipMemsetAsync(ms->mask + (size_t)i * ms->col_stride, 0, (size_t)ms->col_stride * 4, h->stream) != hipSuccess)
            return drained(h, fail(OWW_EHIP, "%s: clearing the hit mask failed", fn));
        const int rc = sw.each(h, h->bank[ids[i]].T, [&](int64_t first, int64_t n) {
            if (int r = ext.score(ids[i], sw.d_slab, n)) return r;
            const float* d_sc = ext.d_sc;
            if (ms) { launch_hits_slab(h, *ms, d_sc, 1, 0, i, nw, first, n); return 0; }
            owh::BankSlabParams sp{};
            sp.scores = d_sc; sp.n_win = nw; sp.first = first; sp.n = n; sp.out = d_out; sp.n_ids = n_ids; sp.col = i;
            sp.thr = thr ? thr[i] : 0.5f; sp.count = d_count; sp.key = d_key;
            {
                Timed t(h, 7);
                hipLaunchKernelGGL(owh::dense_bank_slab_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, sp);
            }
            return 0;
        });
        if (rc) return drained(h, rc);
    }
    if (hipGetLastError() != hipSuccess) return drained(h, fail(OWW_EHIP, "%s: a fallback launch failed", fn));
    return drained(h, 0);           // (the slab and the lists go with this scope)
}

// The device side of a dense entry's features and score matrix: the caller's buffer where it is on the device, a copy owned here
// where it is not.  The matrix entries use open() and finish(); oww_bank_score_stats, whose outputs are its own, the features half.
struct DenseIO {
    oww_ctx* h; const char* fn;
    DevBuf<float> d_f, d_o;
    const float* feats = nullptr; float* out = nullptr;     // on the device
    float* host_out = nullptr; uint64_t ob = 0;             // where `out` goes in the end (nullptr: it is the caller's already)
    // src on the device is used as it is; else a buffer of fb bytes, which upload() fills from src.  True = out of device memory.
    bool alloc_feats(const float* src, int on_device, uint64_t fb) {
        if (!on_device && d_f.alloc(fb / 4)) return true;
        feats = on_device ? src : d_f.get();
        return false;
    }
    hipError_t upload(const float* src, uint64_t fb) { return src != feats ? copy_async(d_f, src, fb, hipMemcpyHostToDevice, h->stream) : hipSuccess; }
    // both buffers, and the features on their way in (src == nullptr: a buffer that the caller fills)
    int open(const float* src, int src_on_device, uint64_t fb, float* dst, int dst_on_device, uint64_t ob_) {
        if (alloc_feats(src, src_on_device, fb) || (!dst_on_device && d_o.alloc(ob_ / 4)))
            return fail(OWW_ENOMEM, "%s: out of device memory (%llu bytes of features, %llu bytes of scores)", fn, (unsigned long long)fb, (unsigned long long)ob_);
        out = dst_on_device ? dst : d_o.get(); host_out = dst_on_device ? nullptr : dst; ob = ob_;
        if (src && upload(src, fb) != hipSuccess) return drained(h, fail(OWW_EHIP, "%s: H2D failed", fn));
        return 0;
    }
    // the matrix on its way out; then the end of the call (oww_score_clips copies its embeddings between the two)
    int download() { return host_out && copy_async(host_out, d_o, ob, hipMemcpyDeviceToHost, h->stream) != hipSuccess ? drained(h, fail(OWW_EHIP, "%s: D2H failed", fn)) : 0; }
    int settle() { return hipStreamSynchronize(h->stream) != hipSuccess ? fail(OWW_EHIP, "%s: device error: %s", fn, hipGetErrorString(hipGetLastError())) : range_check(h, fn); }
    int finish() { const int rc = download(); return rc ? rc : settle(); }
};

// ---- ordered hit lists (oww_score_hits, oww_score_clip_hits, oww_bank_score_hits; owwhip_dense.h, owwhip_dense_hits_host.h) -----------
// One call: (1) the heads launches of the matrix entries in MASK mode (score_device / bank_score_device with a MaskSink) leave one bit
// per (column, sequence, window); (2) dense_hits_compact_kernel, one workgroup per column, turns the bits into ordered records and
// totals; (3) for the stored hits alone, slab by slab: the head's own rows gathered by record (dense_hits_gather_kernel), re-scored as
// external features by the kernels the fallback launches -- the bits of the matrix entry -- the scores written into the records, the
// slab copied out as the hits' windows.  A call without hits ends after (2).
struct HitsBuf {
    int64_t nw = 0, cap = 0, cap_dev = 0;
    DevBuf<unsigned> d_mask; DevBuf<int4> d_hits; DevBuf<unsigned long long> d_total; DevBuf<float> d_thr;
    MaskSink ms{};
};
// the call's device buffers, thresholds up.  The mask is not cleared here: a sliding launch overwrites every word of its columns, and
// score_device / bank_score_device clear the columns that take the fallback, whose bits are ORed in.
int hits_open(oww_ctx* h, const char* fn, int B, int64_t nw, int n_cols, int64_t cap, const std::vector<float>& thr, HitsBuf& hb) {
    hb.nw = nw; hb.cap = cap; hb.cap_dev = owdh::cap_eff(cap, B, nw);
    const int64_t cs = owdh::col_stride(B, nw);
    const uint64_t mb = owdh::mask_bytes(n_cols, B, nw), rb = owdh::hits_bytes(n_cols, hb.cap_dev);
    if (hb.d_mask.alloc((size_t)(mb / 4)) || hb.d_hits.alloc((size_t)(rb / 16)) || hb.d_total.alloc((size_t)n_cols) || hb.d_thr.alloc((size_t)n_cols))
        return fail(OWW_ENOMEM, "%s: out of device memory (%llu bytes of hit mask, %llu bytes of hit records)", fn, (unsigned long long)mb, (unsigned long long)rb);
    if (copy_async(hb.d_thr, thr.data(), thr.size() * sizeof(float), hipMemcpyHostToDevice, h->stream) != hipSuccess) return drained(h, fail(OWW_EHIP, "%s: H2D failed", fn));
    hb.ms = MaskSink{hb.d_mask, cs, owdh::words_per_seq(nw), hb.d_thr, thr.data()};
    return 0;
}
// scores n gathered windows of column c; says where the scores are (score of window i at sc[i * stride + off])
struct HitRescorer {
    virtual ~HitRescorer() = default;
    virtual int prepare(int64_t max_windows) = 0;
    virtual int score(int c, const float* d_slab, int64_t n, const float*& sc, int& stride, int& off) = 0;
};
// steps (2) and (3).  T[c]: the window length of column c's head.
int hits_finish(oww_ctx* h, const char* fn, const float* d_feats, int B, int n_rows, int t_max, int n_cols, const std::vector<int>& T, HitsBuf& hb,
                HitRescorer& rs, oww_dense_hit* hits, int32_t* n_stored, int64_t* n_total, float* windows, int windows_on_device) {
    {
        owh::HitCompactParams cp{};
        cp.mask = hb.d_mask; cp.col_stride = hb.ms.col_stride; cp.wps = hb.ms.wps; cp.B = B; cp.cap = (int)hb.cap_dev; cp.hits = hb.d_hits; cp.total = hb.d_total;
        Timed t(h, 7);
        hipLaunchKernelGGL(owh::dense_hits_compact_kernel, dim3((unsigned)n_cols), dim3(256), 0, h->stream, cp);
    }
    std::vector<unsigned long long> total((size_t)n_cols);
    hipError_t err = hipGetLastError();
    if (err == hipSuccess) err = copy_async(total.data(), hb.d_total, total.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(h->stream);
    if (err != hipSuccess) return drained(h, fail(OWW_EHIP, "%s: device error: %s", fn, hipGetErrorString(err)));
    const int64_t budget = dense_env().budget;
    int64_t slab_bytes = 0, slab_windows = 0;
    for (int c = 0; c < n_cols; ++c) {
        n_total[c] = (int64_t)total[(size_t)c];
        n_stored[c] = (int32_t)std::min<int64_t>(n_total[c], hb.cap);
        if (!n_stored[c]) continue;
        const owd::Slab sl = owd::slab(n_stored[c], T[(size_t)c], budget);
        slab_bytes = std::max(slab_bytes, sl.bytes); slab_windows = std::max(slab_windows, sl.windows);
    }
    if (!slab_bytes) return range_check(h, fn);         // no hits: no gather, no re-score
    DevBuf<float> d_slab;
    if (d_slab.alloc((size_t)slab_bytes / sizeof(float))) return fail(OWW_ENOMEM, "%s: out of device memory (%lld bytes of hit-window slab)", fn, (long long)slab_bytes);
    if (int rc = rs.prepare(slab_windows)) return drained(h, rc);
    std::vector<int64_t> win_offset((size_t)n_cols + 1);
    owdh::win_offsets(T.data(), n_cols, hb.cap, win_offset.data());
    for (int c = 0; c < n_cols; ++c) {
        if (!n_stored[c]) continue;
        const int Tc = T[(size_t)c];
        int4* col_hits = hb.d_hits + (size_t)c * hb.cap_dev;
        for (const owdh::HitSlab& sl : owdh::slab_plan(n_stored[c], Tc, budget)) {
            owh::HitGatherParams gp{};
            gp.feats = d_feats + (size_t)owd::row_offset(t_max, Tc) * 96; gp.seq_stride = (long long)n_rows * 96;
            gp.hits = col_hits + sl.first; gp.n = sl.n; gp.T = Tc; gp.slab = d_slab;
            {
                Timed t(h, 7);
                const int64_t pieces = sl.n * Tc * 24;
                hipLaunchKernelGGL(owh::dense_hits_gather_kernel, dim3((unsigned)std::min<int64_t>((pieces + 255) / 256, 256 * 16)), dim3(256), 0, h->stream, gp);
            }
            owh::HitScoreParams sp{};
            if (int rc = rs.score(c, d_slab, sl.n, sp.scores, sp.stride, sp.off)) return drained(h, rc);
            sp.n = sl.n; sp.hits = col_hits + sl.first;
            {
                Timed t(h, 7);
                hipLaunchKernelGGL(owh::dense_hits_score_kernel, dim3((unsigned)((sl.n + 255) / 256)), dim3(256), 0, h->stream, sp);
            }
            if (windows && copy_async(windows + win_offset[(size_t)c] + sl.first * Tc * 96, d_slab.get(), (size_t)sl.n * Tc * 96 * sizeof(float),
                                      windows_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream) != hipSuccess)
                return drained(h, fail(OWW_EHIP, "%s: window copy failed", fn));
        }
        if (copy_async(hits + (size_t)c * hb.cap, col_hits, (size_t)n_stored[c] * sizeof(oww_dense_hit), hipMemcpyDeviceToHost, h->stream) != hipSuccess)
            return drained(h, fail(OWW_EHIP, "%s: D2H failed", fn));
    }
    if (hipGetLastError() != hipSuccess) return drained(h, fail(OWW_EHIP, "%s: a hit-list launch failed", fn));
    if (hipStreamSynchronize(h->stream) != hipSuccess) return fail(OWW_EHIP, "%s: device error: %s", fn, hipGetErrorString(hipGetLastError()));
    return range_check(h, fn);
}
static_assert(sizeof(oww_dense_hit) == sizeof(int4) && sizeof(oww_dense_hit) == owdh::kHitBytes, "a record is one 16-byte store");

// fixed heads: run_heads on the slab for the column's head (its whole group on the MFMA families; a gated head's two nets with it)
struct FixedRescorer : HitRescorer {
    oww_ctx* h; const char* fn; std::vector<int> col_head; DevBuf<float> d_scr;
    int prepare(int64_t max_windows) override {
        return d_scr.alloc((size_t)max_windows * h->NL) ? fail(OWW_ENOMEM, "%s: out of device memory (%lld bytes of slab scores)", fn, (long long)max_windows * h->NL * 4) : 0;
    }
    int score(int c, const float* d_slab, int64_t n, const float*& sc, int& stride, int& off) override {
        sc = d_scr; stride = h->NL; off = c;
        return run_heads(h, step_args(h), (int)n, false, d_slab, col_head[(size_t)c], d_scr, 0);
    }
};
// the fixed columns of a handle: T and head of every column
void fixed_columns(const oww_ctx* h, std::vector<int>& T, std::vector<int>& head) {
    T.assign((size_t)h->NL, 0); head.assign((size_t)h->NL, 0);
    for (size_t hi = 0; hi < h->heads.size(); ++hi)
        for (int o = 0; o < h->heads[hi].n_out; ++o) { T[(size_t)(h->heads[hi].out_col + o)] = h->heads[hi].T; head[(size_t)(h->heads[hi].out_col + o)] = (int)hi; }
}
// bank heads: bank_score_device's fallback launch (BankExtScorer) on the gathered hits
struct BankRescorer : HitRescorer {
    BankExtScorer ext; const int32_t* ids;
    BankRescorer(oww_ctx* h, const char* fn, const int32_t* ids_) : ext{h, fn}, ids(ids_) {}
    int prepare(int64_t max_windows) override { return ext.prepare(max_windows); }
    int score(int c, const float* d_slab, int64_t n, const float*& sc, int& stride, int& off) override {
        sc = ext.d_sc; stride = 1; off = 0;
        return ext.score(ids[c], d_slab, n);
    }
};

// the features half of a fixed-heads hit-list call, shared by oww_score_hits and oww_score_clip_hits: d_feats [B][n_rows][96] on the device
int score_hits_device(oww_ctx* h, const char* fn, const float* d_feats, int B, int n_rows, const float* thresholds, int32_t cap, oww_dense_hit* hits,
                      int32_t* n_stored, int64_t* n_total, float* windows, int windows_on_device) {
    const int t_max = dense_t_max(h);
    std::vector<float> thr((size_t)h->NL, 0.5f);                // train.py:100's default
    if (thresholds) thr.assign(thresholds, thresholds + h->NL);
    HitsBuf hb;
    if (int rc = hits_open(h, fn, B, owd::n_win(n_rows, t_max), h->NL, cap, thr, hb)) return rc;
    if (int rc = score_device(h, fn, d_feats, B, n_rows, nullptr, &hb.ms)) return drained(h, rc);
    FixedRescorer rs; rs.h = h; rs.fn = fn;
    std::vector<int> T;
    fixed_columns(h, T, rs.col_head);
    return hits_finish(h, fn, d_feats, B, n_rows, t_max, h->NL, T, hb, rs, hits, n_stored, n_total, windows, windows_on_device);
}

}  // namespace

extern "C" {

int oww_abi_version(void) { return OWW_ABI_VERSION; }
#ifndef OWW_SRC_SHA16
#define OWW_SRC_SHA16 "unknown"            /* (set by openwakeword_amd/_build.py: hash of csrc/ + include/owwhip.h) */
#endif
const char* oww_build_info(void) { return "src=" OWW_SRC_SHA16 " arch=gfx950"; }
const char* oww_last_error(void) { return g_err.c_str(); }

int oww_create(const oww_config* cfg, oww_ctx** out) {
    OWW_GUARD_BEGIN
    if (!cfg || !out) return fail(OWW_EINVAL, "oww_create: null argument");
    if (cfg->n_streams < 1) return fail(OWW_EINVAL, "oww_create: n_streams must be >= 1");
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (cfg->device < 0 || cfg->device >= ndev) return fail(OWW_EINVAL, "oww_create: device %d of %d", cfg->device, ndev);
    HIPCHK(hipSetDevice(cfg->device));
    oww_ctx* h = new (std::nothrow) oww_ctx();
    if (!h) return fail(OWW_ENOMEM, "oww_create: out of host memory");
    h->cfg = *cfg;
    h->S = cfg->n_streams;
    h->Spad = (h->S + 31) / 32 * 32;
    h->kmax = std::max(1, cfg->max_chunks);
    h->mfma = cfg->use_mfma != 0;
    h->rr = cfg->use_mfma == 1 || cfg->use_mfma == 3;
    h->hx = cfg->use_mfma == 3;
    h->state_len = h->rr ? kStateLenRr : kStateLenLds;
    if (cfg->stream) h->stream.borrow(reinterpret_cast<hipStream_t>(cfg->stream));      // (the caller's: never destroyed)
    else if (const int e = h->stream.create(hipStreamNonBlocking)) { delete h; return fail(OWW_EHIP, "hipStreamCreate: %s", hipGetErrorString(herr(e))); }
    *out = h;
    return OWW_OK;
    OWW_GUARD_END
}

int oww_destroy(oww_ctx* h) {
    OWW_GUARD_BEGIN
    if (!h) return OWW_OK;
    (void)hipSetDevice(h->cfg.device);
    delete h;                                    // (~oww_ctx drains the handle's streams before anything is released)
    return OWW_OK;
    OWW_GUARD_END
}

int oww_load_mel(oww_ctx* h, const void* blob, size_t nbytes) {
    OWW_GUARD_BEGIN
    if (!h || !blob) return fail(OWW_EINVAL, "oww_load_mel: null argument");
    if (h->committed) return fail(OWW_ESTATE, "weights already committed");
    return parse_mel_blob(blob, nbytes, h->mel_blob);
    OWW_GUARD_END
}

int oww_load_embedding(oww_ctx* h, const void* blob, size_t nbytes) {
    OWW_GUARD_BEGIN
    if (!h || !blob) return fail(OWW_EINVAL, "oww_load_embedding: null argument");
    if (h->committed) return fail(OWW_ESTATE, "weights already committed");
    return parse_embedding_blob(blob, nbytes, h->emb_blob);
    OWW_GUARD_END
}

int oww_add_head(oww_ctx* h, const void* blob, size_t nbytes) {
    OWW_GUARD_BEGIN
    if (!h || !blob || nbytes < 32) return fail(OWW_EINVAL, "oww_add_head: bad argument");
    if (h->committed) return fail(OWW_ESTATE, "weights already committed");
    if ((int)h->heads.size() >= OWW_MAX_HEADS) return fail(OWW_EINVAL, "too many heads");
    HeadHost hh{};
    if (int rc = parse_head_blob("oww_add_head", blob, nbytes, 120, hh)) return rc;
    h->heads.push_back(std::move(hh));
    return (int)h->heads.size() - 1;
    OWW_GUARD_END
}

int oww_load_vad(oww_ctx* h, const void* blob, size_t nbytes) {
    OWW_GUARD_BEGIN
    if (!h || !blob) return fail(OWW_EINVAL, "oww_load_vad: null argument");
    if (h->committed) return fail(OWW_ESTATE, "weights already committed");
    return parse_vad_blob(blob, nbytes, h->vad_blob);
    OWW_GUARD_END
}

int oww_set_calibration(oww_ctx* h, const int16_t* pcm, int32_t n_streams, int32_t n_frames) {
    OWW_GUARD_BEGIN
    if (!h) return fail(OWW_EINVAL, "oww_set_calibration: null handle");
    if (h->committed) return fail(OWW_ESTATE, "oww_set_calibration: call before oww_commit");
    h->cal_user.clear();
    if (!pcm || n_streams < 1 || n_frames < 1) return OWW_OK;          // (clears the set)
    const size_t seg = (size_t)CAL_T * OWW_CHUNK;
    const int per = (n_frames + CAL_T - 1) / CAL_T;                     // CAL_T-frame segments per stream (the last one zero-padded)
    const size_t n_seg = std::min<size_t>((size_t)n_streams * per, (size_t)(CAL_MAX_BATCHES - 1) * CAL_NP);
    h->cal_user.assign(n_seg * seg, 0);
    for (size_t k = 0; k < n_seg; ++k) {
        const size_t s = k / per, part = k % per;
        const size_t first = part * seg, n = std::min(seg, (size_t)n_frames * OWW_CHUNK - first);
        memcpy(&h->cal_user[k * seg], pcm + s * (size_t)n_frames * OWW_CHUNK + first, n * sizeof(int16_t));
    }
    return OWW_OK;
    OWW_GUARD_END
}

int oww_calibration_info(oww_ctx* h, float absmax[20], int32_t exps[21], int32_t* n_probe_streams, float selftest[3]) {
    OWW_GUARD_BEGIN
    if (!h || !h->committed) return fail(OWW_ESTATE, "oww_calibration_info: handle not committed");
    if (!h->hx) return fail(OWW_ESTATE, "oww_calibration_info: only the fp16-split family (use_mfma = 3) calibrates");
    if (absmax) memcpy(absmax, h->hx_absmax, sizeof h->hx_absmax);
    if (exps) { for (int l = 0; l < 20; ++l) exps[l] = h->hx_e[l]; exps[20] = h->hx_efeat; }
    if (n_probe_streams) *n_probe_streams = CAL_NP + (int32_t)(h->cal_user.size() / ((size_t)CAL_T * OWW_CHUNK));
    if (selftest) { selftest[0] = h->hx_selftest_err; selftest[1] = h->hx_selftest_ref; selftest[2] = h->hx_selftest_score_err; }
    return OWW_OK;
    OWW_GUARD_END
}

int oww_n_labels(const oww_ctx* h) { return h ? h->NL : 0; }

int oww_commit(oww_ctx* h) {
    OWW_GUARD_BEGIN
    if (!h) return fail(OWW_EINVAL, "null handle");
    if (h->committed) return fail(OWW_ESTATE, "already committed");
    if (h->mel_blob.empty() || h->emb_blob.empty()) return fail(OWW_ESTATE, "mel and embedding weights must be loaded before commit");
    HIPCHK(hipSetDevice(h->cfg.device));
    h->feature_ring = h->cfg.feature_ring;
    if (int rc = build_nets(*h, h->NL, h->TR, h->generic_hmax)) return rc;
    if (h->evt_rows > h->TR)                     // (the ring is known only now)
        return fail(OWW_EINVAL, "oww_events_configure: feature_rows = %d exceeds the handle's feature ring (%d rows)", h->evt_rows, h->TR);
    if (int rc = owa::commit_check(h->aud_evt, h->evt_cap)) return rc;
    // ---- f16-split family: per-layer activation scales from a calibration run on the exact-fp32 kernels (calibrate_hx) ----
    CommitClock clk(h->hx ? "f16-split" : "family");
    HxCalib cal;
    if (h->hx) {
        if (int rc = calibrate_hx(h, cal)) return rc;
        h->probe_emb = cal.ref_emb; h->probe_nb = cal.nb;                  // (hx_hidden_exp's and oww_bank_add's self-test inputs)
        clk.lap("calibration (total)");
        if (getenv("OWW_DEBUG_CALIB"))
            for (int l = 0; l < 20; ++l) fprintf(stderr, "calib layer %2d: max|a| %-12.5g e_in %4d e_out %4d\n", l, h->hx_absmax[l], h->hx_ein[l], h->hx_e[l]);
    }
    // ---- device weight image: pack, upload ----
    HostBuf hb;
    WeightOff off;
    HeadGroups hg;
    h->no_wide_heads = getenv("OWW_NO_WIDE_HEADS") != nullptr;
    if (int rc = pack_mel_tables(*h, hb, off)) return rc;
    if (int rc = pack_cnn(*h, hb, off)) return rc;
    pack_net_arrays(*h, hb, off);
    if (int rc = pack_head_groups(*h, hg, hb, off)) return rc;
    h->groups.clear();
    for (const HeadGroup& g : hg.groups) h->groups.push_back(FastGroup{g});
    h->generic_nets = hg.generic_nets; h->rnn_nets = hg.rnn_nets;
    h->vad = !h->vad_blob.empty();
    if (int rc = pack_vad(*h, hb, off, h->vad_gain, h->vad_bd)) return rc;
    clk.lap("weight packing (host)");
    if (int rc = bind_weights(h, hb, off)) return rc;
    if (int rc = alloc_range_flag(h)) return rc;
    clk.lap("weight upload");
    // ---- state ----
    if (int rc = alloc_state(h)) return rc;
    h->fuse = h->hx && !getenv("OWW_NO_FUSE");                            // (A/B switch: OWW_NO_FUSE=1 keeps the separate mel kernel)
    if (const char* e = getenv("OWW_SMALL_WGS")) h->small_wgs = atoi(e);
    if (const char* e = getenv("OWW_SMALL_WGS_HEADS")) h->small_wgs_heads = atoi(e);
    if (const char* e = getenv("OWW_RESIDENT_B")) h->resident_b = strcmp(e, "auto") == 0 ? -1 : (atoi(e) != 0 ? 1 : 0);
    if (const char* e = getenv("OWW_RESIDENT_B_WGS")) h->resident_b_wgs = std::max(1, atoi(e));
    if (const char* e = getenv("OWW_GENERIC_SPW")) { const int v = atoi(e); h->generic_spw = v == 4 || v == 16 ? v : 0; }
    h->post_in_heads = h->fuse && h->groups.size() == 1 && h->groups[0].ht == 4 && h->generic_nets.empty() && h->rnn_nets.empty() && h->NL > 0;
    if (int rc = set_kernel_lds(h)) return rc;
    clk.lap("state allocation");
    // ---- reset state, then reset all ----
    if (int rc = derive_reset_state(h, cal, clk)) return rc;
    if (h->bank_K > 0) if (int rc = alloc_bank(h)) return rc;
    if (h->vpool_cap > 0) if (int rc = alloc_verifiers(h)) return rc;
    if (audio_on(h)) if (int rc = alloc_audio(h)) return rc;
    if (events_on(h)) if (int rc = alloc_events(h)) return rc;
    h->committed = true;
    return OWW_OK;
    OWW_GUARD_END
}

int oww_reset(oww_ctx* h, const int32_t* stream_ids, int32_t n, const float* init_features) {
    OWW_GUARD_BEGIN
    if (!h || !h->committed) return fail(OWW_ESTATE, "oww_reset: handle not committed");
    HIPCHK(hipSetDevice(h->cfg.device));
    const float* d_init = nullptr;
    if (init_features) {
        HIPCHK(copy_async(h->d_featinit, init_features, (size_t)h->TR * 96 * sizeof(float), hipMemcpyHostToDevice, h->stream));
        d_init = h->d_featinit;
    }
    if (!stream_ids) {
        if (int rc = do_reset(h, nullptr, h->Spad, d_init)) return rc;
    } else {
        if (n < 1) return OWW_OK;
        for (int i = 0; i < n; ++i)
            if (stream_ids[i] < 0 || stream_ids[i] >= h->S) return fail(OWW_EINVAL, "oww_reset: stream id %d out of range", stream_ids[i]);
        if (int rc = upload_ids(h, stream_ids, n)) return rc;
        if (int rc = do_reset(h, h->d_ids, n, d_init)) return rc;
    }
    if (h->ing.ready && h->ing.tab.Hpad_max) {   // stateful ingest: a new caller starts from silence
        hipLaunchKernelGGL(ingest_hist_reset_kernel, dim3(stream_ids ? n : h->S), dim3(64), 0, h->stream, h->ing.d_hist, h->ing.tab.Hpad_max,
                           stream_ids ? h->d_ids : nullptr, stream_ids ? n : h->S);
        HIPCHK(hipGetLastError());
    }
    if (audio_on(h)) if (int rc = audio_reset(h, stream_ids ? (const int*)h->d_ids : nullptr, n)) return rc;   // utils.py:174
    std::vector<int> slots;                      // head bank: Model.reset() empties every prediction buffer, the subscriptions stay
    if (h->bank_K > 0) {
        if (!stream_ids) for (int i = 0; i < h->S * h->bank_K; ++i) slots.push_back(i);
        else for (int i = 0; i < n; ++i) for (int k = 0; k < h->bank_K; ++k) slots.push_back(stream_ids[i] * h->bank_K + k);
        if (int rc = bank_clear(h, slots)) return rc;
    }
    HIPCHK(hipStreamSynchronize(h->stream));     // host buffers may be reused by the caller
    return OWW_OK;
    OWW_GUARD_END
}

int oww_set_postproc(oww_ctx* h, const int32_t* patience, const float* threshold, int32_t debounce_frames) {
    OWW_GUARD_BEGIN
    if (!h || !h->committed) return fail(OWW_ESTATE, "oww_set_postproc: handle not committed");
    HIPCHK(hipSetDevice(h->cfg.device));
    std::vector<int> pat(std::max(h->NL, 1), 0);
    std::vector<float> thr(std::max(h->NL, 1), NAN);
    if (patience) for (int i = 0; i < h->NL; ++i) pat[i] = patience[i];
    if (threshold) for (int i = 0; i < h->NL; ++i) thr[i] = threshold[i];
    HIPCHK(copy_async(h->d_patience, pat.data(), pat.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(copy_async(h->d_threshold, thr.data(), thr.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->debounce_frames = debounce_frames;
    if (h->graph_exec) { (void)hipGraphExecDestroy(h->graph_exec); h->graph_exec = nullptr; }   // baked-in scalar changed
    return OWW_OK;
    OWW_GUARD_END
}

int oww_step(oww_ctx* h, const int16_t* pcm, int pcm_on_device, int32_t n_chunks, float* scores, int scores_on_device) {
    OWW_GUARD_BEGIN
    if (!h || !h->committed) return fail(OWW_ESTATE, "oww_step: handle not committed");
    if (!pcm) return fail(OWW_EINVAL, "oww_step: pcm is null");
    if (n_chunks < 1 || n_chunks > OWW_MAX_CALL_CHUNKS) return fail(OWW_EINVAL, "oww_step: n_chunks=%d outside [1,%d]", n_chunks, OWW_MAX_CALL_CHUNKS);
    if (int rc = range_check(h, "oww_step")) return rc;          // raised by an earlier (asynchronous) step: sticky
    HIPCHK(hipSetDevice(h->cfg.device));
    h->k_last = n_chunks;
    const StepArgs a = step_args(h);
    const size_t n_pcm = (size_t)h->S * OWW_CHUNK * n_chunks;
    if (n_chunks > h->kmax) {                                    // longer than the mel buffer: slices that share the call's clamp floor
        const int16_t* d_call = pcm;
        if (!pcm_on_device) {
            if (grow(h, h->d_long, n_pcm) != hipSuccess) return fail(OWW_ENOMEM, "oww_step: out of device memory for a call of %d chunks", n_chunks);
            HIPCHK(copy_async(h->d_long, pcm, n_pcm * sizeof(int16_t), hipMemcpyHostToDevice, h->stream));
            d_call = h->d_long;
        }
        if (int rc = launch_step_long(h, a, d_call, n_chunks)) return rc;
        if (audio_on(h)) if (int rc = launch_audio_append(h, a, d_call, n_chunks)) return rc;
        if (events_on(h)) { if (int rc = launch_events(h, a, h->evt_sync)) return rc; h->evt_cur = &h->evt_sync; }
        // (host PCM: the caller's buffer is free to change when this returns)
        return deliver_scores(h, scores, scores_on_device, !scores_on_device || !pcm_on_device, "oww_step");
    }
    const bool graphable = h->want_graph && n_chunks == 1 && !h->timing;
    const int16_t* d_pcm = pcm;
    if (!pcm_on_device || graphable) {
        HIPCHK(copy_async(h->d_pcm, pcm, n_pcm * sizeof(int16_t), pcm_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
        d_pcm = h->d_pcm;
    }
    if (graphable) {
        if (!h->graph_exec) {
            HIPCHK(hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
            const int rc = launch_step(h, a, h->d_pcm, 1);
            hipGraph_t g = nullptr;
            const hipError_t e = hipStreamEndCapture(h->stream, &g);
            if (rc) return rc;
            if (e != hipSuccess) return fail(OWW_EHIP, "hipStreamEndCapture: %s", hipGetErrorString(e));
            if (h->graph) (void)hipGraphDestroy(h->graph);
            h->graph = g;
            HIPCHK(hipGraphInstantiate(&h->graph_exec, h->graph, nullptr, nullptr, 0));
        }
        HIPCHK(hipGraphLaunch(h->graph_exec, h->stream));
    } else {
        if (int rc = launch_step(h, a, d_pcm, n_chunks)) return rc;
    }
    if (audio_on(h)) if (int rc = launch_audio_append(h, a, d_pcm, n_chunks)) return rc;
    if (events_on(h)) { if (int rc = launch_events(h, a, h->evt_sync)) return rc; h->evt_cur = &h->evt_sync; }
    return deliver_scores(h, scores, scores_on_device, scores && !scores_on_device, "oww_step");
    OWW_GUARD_END
}

int oww_step_masked(oww_ctx* h, const int16_t* pcm, int pcm_on_device, const uint8_t* stream_on, int stream_on_on_device,
                    float* scores, int scores_on_device) {
    OWW_GUARD_BEGIN
    if (!h || !h->committed) return fail(OWW_ESTATE, "oww_step_masked: handle not committed");
    if (!pcm || !stream_on) return fail(OWW_EINVAL, "oww_step_masked: null argument");
    if (!h->rr) return fail(OWW_EINVAL, "oww_step_masked: needs the register-resident kernel families (use_mfma = 3 or 1)");
    if (int rc = range_check(h, "oww_step_masked")) return rc;
    HIPCHK(hipSetDevice(h->cfg.device));
    h->k_last = 1;
    if (int rc = ensure_mask(h)) return rc;
    HIPCHK(copy_async(h->d_on, stream_on, h->S, stream_on_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
    const int16_t* d_pcm = pcm;
    if (!pcm_on_device || (reinterpret_cast<uintptr_t>(pcm) & 15)) {
        HIPCHK(copy_async(h->d_pcm, pcm, (size_t)h->S * OWW_CHUNK * sizeof(int16_t),
                              pcm_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
        d_pcm = h->d_pcm;
    }
    StepArgs a = step_args(h);
    a.on = h->d_on;
    int n_act = -1;
    if (!stream_on_on_device) {                                 // few participants: only their groups are launched (build_active_lists)
        n_act = build_active_lists(h, stream_on, a);
        if (n_act < -1) return n_act + 100;
    }
    if (n_act != 0)                                             // (nobody takes part: nothing moves)
        if (int rc = launch_step(h, a, d_pcm, 1)) return rc;
    if (audio_on(h)) if (int rc = launch_audio_append(h, a, d_pcm, 1, n_act != 0)) return rc;
    if (events_on(h)) { if (int rc = launch_events(h, a, h->evt_sync, n_act != 0)) return rc; h->evt_cur = &h->evt_sync; }
    return deliver_scores(h, scores, scores_on_device, scores && !scores_on_device, "oww_step_masked");
    OWW_GUARD_END
}

static int ensure_ingest(oww_ctx* h) {
    if (h->up_stream) return 0;
    HIPCHK(herr(h->up_stream.create(hipStreamNonBlocking)));
    HIPCHK(herr(h->down_stream.create(hipStreamNonBlocking)));
    const size_t n_sc = (size_t)h->S * std::max(h->NL, 1);
    for (auto& sl : h->slot) {
        HIPCHK(herr(sl.d_pcm.alloc((size_t)h->S * OWW_CHUNK * h->kmax)));
        HIPCHK(herr(sl.d_scores.alloc(n_sc)));
        HIPCHK(herr(sl.h_scores.alloc(n_sc, hipHostMallocDefault)));
        HIPCHK(herr(sl.h_on.alloc(h->S, hipHostMallocDefault)));
        for (owm::Event* e : {&sl.up, &sl.done, &sl.down}) HIPCHK(herr(e->create(hipEventDisableTiming)));
    }
    if (events_on(h)) {
        for (auto& b : h->evt_slot) if (int rc = alloc_event_buf(h, b, true)) return rc;
        HIPCHK(hipStreamSynchronize(h->stream));          // (the buffers' zero fill: before the first download reads the counts)
    }
    return 0;
}

// The ingest launch on the handle's stream, the one place where the two forms differ: d_in [S][row_bytes] and d_on (or null) are
// device pointers, `out` is a device pointer, `g` is what single_check / mixed_check gave for this message.  A single-format handle
// has a kernel of its own (the class kernel serves one class slower).
static_assert(owi::kTile == IG_TILE && sizeof(owi::ClassDev) == sizeof(IngestClass), "owwhip_ingest.h restates the kernel's tile and table row");
static int launch_ingest(oww_ctx* h, const void* d_in, long long row_bytes, int n_out, const uint8_t* d_on, int16_t* out, const owi::Geometry& g) {
    const oww_ctx::Ingest& ing = h->ing;
    const dim3 grid(h->S), block(RS_NT);
    if (ing.mixed) {
        IngestMixedParams m{};
        m.in = static_cast<const char*>(d_in); m.out = out; m.hist = ing.d_hist; m.taps = ing.d_taps; m.on = d_on;
        m.cls = ing.d_cls; m.table = ing.d_table;
        m.row_bytes = row_bytes; m.n_out = n_out; m.Hpad_max = ing.tab.Hpad_max; m.lds_floats = (int)(g.lds / sizeof(float));
        m.in_aligned = !(reinterpret_cast<uintptr_t>(d_in) & 15);
        m.vec_out = !(reinterpret_cast<uintptr_t>(out) & 15) && n_out % 8 == 0;
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(ingest_mixed_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        hipLaunchKernelGGL(ingest_mixed_kernel, grid, block, g.lds, h->stream, m);
    } else {
        const owi::ClassDev& k = ing.tab.dev[0];
        IngestParams a{};
        a.in = d_in; a.on = d_on; a.out = out; a.hist = ing.d_hist; a.taps = ing.d_taps;
        a.enc = k.enc; a.n_in = (int)((long long)n_out * k.p / k.q); a.n_out = n_out; a.p = k.p; a.q = k.q; a.n_taps = k.n_taps; a.ntp = k.ntp;
        a.Hpad = k.Hpad; a.xs_len = g.xs_len; a.taps_in_lds = g.taps_in_lds;
        a.vec_in = !(reinterpret_cast<uintptr_t>(d_in) & 15) && row_bytes % 16 == 0;
        a.vec_out = !(reinterpret_cast<uintptr_t>(out) & 15) && n_out % 8 == 0;
        a.slide = k.slide;
#define OWW_IG_GO(ENC)                                                                                                                        \
    do {                                                                                                                                      \
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(ingest_kernel<ENC>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)); \
        hipLaunchKernelGGL(ingest_kernel<ENC>, grid, block, g.lds, h->stream, a);                                                            \
    } while (0)
        if (k.enc == OWW_ENC_PCM16) OWW_IG_GO(IG_PCM16); else if (k.enc == OWW_ENC_ULAW) OWW_IG_GO(IG_ULAW); else OWW_IG_GO(IG_ALAW);
#undef OWW_IG_GO
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// what a submit uploads: 16 kHz PCM [S][n_chunks * 1280], or (mix != nullptr; oww_submit_ingest_mixed) one chunk per stream in the
// streams' own formats, [S][row_bytes], checked by the caller, who passes mixed_check's geometry
struct SubmitSource { const int16_t* pcm; int32_t n_chunks; const void* mix; long long row_bytes; owi::Geometry geo; };
static int submit_impl(oww_ctx* h, const SubmitSource& src, const uint8_t* stream_on) {
    const void* mix = src.mix;
    const int32_t n_chunks = src.n_chunks;
    if (!h || !h->committed) return fail(OWW_ESTATE, "oww_submit: handle not committed");
    if (!src.pcm && !mix) return fail(OWW_EINVAL, "oww_submit: pcm is null");
    if (n_chunks < 1 || n_chunks > h->kmax) return fail(OWW_EINVAL, "oww_submit: n_chunks=%d outside [1,%d]", n_chunks, h->kmax);
    if (int rc = range_check(h, "oww_submit")) return rc;
    HIPCHK(hipSetDevice(h->cfg.device));
    h->k_last = n_chunks;
    if (int rc = ensure_ingest(h)) return rc;
    auto& sl = h->slot[h->n_submit & 1];
    if (sl.busy) return fail(OWW_ESTATE, "oww_submit: two steps already in flight, call oww_collect first");
    const size_t n_pcm = (size_t)h->S * OWW_CHUNK * n_chunks;
    if (mix) {
        const size_t nb = (size_t)h->S * (size_t)src.row_bytes;
        if (nb > sl.d_mix.capacity()) {                // first use, or wider rows than before (the slot was collected: nothing reads the old block)
            if (sl.d_mix.reserve(nb)) return fail(OWW_ENOMEM, "oww_submit_ingest_mixed: out of device memory for %zu bytes", nb);
        }
        HIPCHK(copy_async(sl.d_mix, mix, nb, hipMemcpyHostToDevice, h->up_stream));
    } else {
        HIPCHK(copy_async(sl.d_pcm, src.pcm, n_pcm * sizeof(int16_t), hipMemcpyHostToDevice, h->up_stream));
    }
    HIPCHK(hipEventRecord(sl.up, h->up_stream));
    HIPCHK(hipStreamWaitEvent(h->stream, sl.up, 0));
    StepArgs a = step_args(h);
    int n_act = -1;
    if (stream_on) {                                   // (the mask is small: copied on the compute stream, ordered before this step's kernels)
        if (int rc = ensure_mask(h)) return rc;
        memcpy(sl.h_on, stream_on, h->S);              // the caller's array is free again when this call returns
        HIPCHK(copy_async(h->d_on, sl.h_on, h->S, hipMemcpyHostToDevice, h->stream));
        a.on = h->d_on;
        n_act = build_active_lists(h, stream_on, a);
        if (n_act < -1) return n_act + 100;
    }
    if (mix && n_act != 0)                             // (both slots' ingest launches and steps are ordered on the compute stream: one staging buffer)
        if (int rc = launch_ingest(h, sl.d_mix, src.row_bytes, OWW_CHUNK, stream_on ? (const uint8_t*)h->d_on : nullptr, h->ing.d_out, src.geo)) return rc;
    if (n_act != 0)
        if (int rc = launch_step(h, a, mix ? (const int16_t*)h->ing.d_out : (const int16_t*)sl.d_pcm, n_chunks)) return rc;
    if (audio_on(h))                                   // from the slot's own buffer (or the ingest staging), on the compute stream
        if (int rc = launch_audio_append(h, a, mix ? (const int16_t*)h->ing.d_out : (const int16_t*)sl.d_pcm, n_chunks, n_act != 0)) return rc;
    const oww_ctx::EventBuf& eb = h->evt_slot[h->n_submit & 1];
    if (events_on(h)) { if (int rc = launch_events(h, a, eb, n_act != 0)) return rc; h->evt_cur = nullptr; }
    const size_t nb = (size_t)h->S * h->NL * sizeof(float);
    if (nb) HIPCHK(copy_async(sl.d_scores, h->d_scores, nb, hipMemcpyDeviceToDevice, h->stream));   // d_scores is rewritten by the next step
    HIPCHK(hipEventRecord(sl.done, h->stream));
    HIPCHK(hipStreamWaitEvent(h->down_stream, sl.done, 0));
    if (nb) HIPCHK(copy_async(sl.h_scores, sl.d_scores, nb, hipMemcpyDeviceToHost, h->down_stream));
    if (events_on(h)) {           // counts and records behind the scores; the slot's buffers are not reused before its oww_collect
        HIPCHK(copy_async(eb.h_count, eb.d_count, 2 * sizeof(int), hipMemcpyDeviceToHost, h->down_stream));
        HIPCHK(copy_async(eb.h_rec, eb.d_rec, (size_t)h->evt_cap * sizeof(oww_event), hipMemcpyDeviceToHost, h->down_stream));
    }
    HIPCHK(hipEventRecord(sl.down, h->down_stream));
    sl.busy = true;
    ++h->n_submit;
    return OWW_OK;
}

int oww_submit(oww_ctx* h, const int16_t* pcm, int32_t n_chunks) { OWW_GUARD_BEGIN return submit_impl(h, SubmitSource{pcm, n_chunks, nullptr, 0, {}}, nullptr); OWW_GUARD_END }

int oww_submit_masked(oww_ctx* h, const int16_t* pcm, const uint8_t* stream_on) {
    OWW_GUARD_BEGIN
    if (!stream_on) return fail(OWW_EINVAL, "oww_submit_masked: stream_on is null");
    if (h && h->committed && !h->rr)
        return fail(OWW_EINVAL, "oww_submit_masked: needs the register-resident kernel families (use_mfma = 3 or 1; see oww_step_masked)");
    return submit_impl(h, SubmitSource{pcm, 1, nullptr, 0, {}}, stream_on);
    OWW_GUARD_END
}

int oww_collect(oww_ctx* h, float* scores) {
    OWW_GUARD_BEGIN
    if (!h || !h->committed) return fail(OWW_ESTATE, "oww_collect: handle not committed");
    auto& sl = h->slot[h->n_collect & 1];
    if (h->n_collect == h->n_submit || !sl.busy) return fail(OWW_ESTATE, "oww_collect: no step in flight");
    HIPCHK(hipSetDevice(h->cfg.device));
    HIPCHK(hipEventSynchronize(sl.down));
    if (scores) memcpy(scores, sl.h_scores, (size_t)h->S * h->NL * sizeof(float));
    if (events_on(h)) h->evt_cur = &h->evt_slot[h->n_collect & 1];
    sl.busy = false;
    ++h->n_collect;
    if (int rc = range_check(h, "oww_collect")) return rc;      // the step is consumed; its scores are suspect
    return OWW_OK;
    OWW_GUARD_END
}

int oww_host_alloc(void** out, size_t nbytes) {
    OWW_GUARD_BEGIN
    if (!out || !nbytes) return fail(OWW_EINVAL, "oww_host_alloc: bad argument");
    if (owm::pinned_alloc_raw(out, nbytes, hipHostMallocDefault)) { *out = nullptr; return fail(OWW_ENOMEM, "oww_host_alloc: %zu bytes of page-locked memory not available", nbytes); }
    return OWW_OK;
    OWW_GUARD_END
}

int oww_host_free(void* p) {
    OWW_GUARD_BEGIN
    if (p) HIPCHK(herr(owm::pinned_free_raw(p)));
    return OWW_OK;
    OWW_GUARD_END
}

int oww_set_verifier(oww_ctx* h, int32_t label, const float* w, int32_t n_w, float bias, float threshold) {
    OWW_GUARD_BEGIN
    if (!h || !h->committed) return fail(OWW_ESTATE, "oww_set_verifier: handle not committed");
    if (label < 0 || label >= h->NL) return fail(OWW_EINVAL, "oww_set_verifier: label %d outside [0,%d)", label, h->NL);
    HIPCHK(hipSetDevice(h->cfg.device));
    int T = 0;                                         // feature rows of the model that owns this label
    for (const auto& hh : h->heads) if (label >= hh.out_col && label < hh.out_col + hh.n_out) T = hh.T;
    if (w && n_w != T * OWW_EMB_DIM) return fail(OWW_EINVAL, "oww_set_verifier: %d weights given, the label's model has %d x 96 = %d features", n_w, T, T * OWW_EMB_DIM);
    if (w) {                                           // (as oww_verifier_add: a NaN or an infinity would re-score every hit to NaN, 0 or 1)
        for (int i = 0; i < n_w; ++i) if (!std::isfinite(w[i])) return fail(OWW_EINVAL, "oww_set_verifier: weight %d is not finite", i);
        if (!std::isfinite(bias)) return fail(OWW_EINVAL, "oww_set_verifier: the bias is not finite");
    }
    if (!h->d_verw) {
        int maxT = 1;
        for (const auto& hh : h->heads) maxT = std::max(maxT, hh.T);
        h->ver_stride = maxT * OWW_EMB_DIM;
        if (int rc = dalloc(h->stream, h->d_verw, (size_t)h->NL * h->ver_stride)) return rc;
        if (int rc = dalloc(h->stream, h->d_verb, (size_t)h->NL)) return rc;
        if (int rc = dalloc(h->stream, h->d_verthr, (size_t)h->NL)) return rc;
        if (int rc = dalloc(h->stream, h->d_verT, (size_t)h->NL)) return rc;
        h->ver_T.assign(h->NL, 0);
        h->ver_thr.assign(h->NL, 0.f);
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    if (w) {
        HIPCHK(copy_sync(h->d_verw + (size_t)label * h->ver_stride, w, (size_t)n_w * sizeof(float), hipMemcpyHostToDevice));
        HIPCHK(copy_sync(h->d_verb + label, &bias, sizeof(float), hipMemcpyHostToDevice));
        HIPCHK(copy_sync(h->d_verthr + label, &threshold, sizeof(float), hipMemcpyHostToDevice));
        h->ver_thr[label] = threshold;
    }
    h->ver_T[label] = w ? T : 0;
    HIPCHK(copy_sync(h->d_verT, h->ver_T.data(), (size_t)h->NL * sizeof(int), hipMemcpyHostToDevice));
    h->n_verifiers = 0;
    for (int t : h->ver_T) h->n_verifiers += t > 0;
    if (h->graph_exec) { (void)hipGraphExecDestroy(h->graph_exec); h->graph_exec = nullptr; }       // the launch list changed
    if (sv_active(h)) if (int rc = sv_rebuild(h)) return rc;     // the pairs at the default follow the handle-wide verifier
    return OWW_OK;
    OWW_GUARD_END
}

int oww_set_vad_threshold(oww_ctx* h, float threshold) {
    OWW_GUARD_BEGIN
    if (!h || !h->committed) return fail(OWW_ESTATE, "oww_set_vad_threshold: handle not committed");
    if (!(threshold == threshold)) return fail(OWW_EINVAL, "oww_set_vad_threshold: NaN");
    h->vad_threshold = threshold;
    if (h->graph_exec) { (void)hipGraphExecDestroy(h->graph_exec); h->graph_exec = nullptr; }     // the threshold is a kernel argument
    return OWW_OK;
    OWW_GUARD_END
}

int oww_push_vad(oww_ctx* h, const float* vad_scores, int on_device) {
    OWW_GUARD_BEGIN
    if (!h || !h->committed) return fail(OWW_ESTATE, "oww_push_vad: handle not committed");
    if (!vad_scores) return fail(OWW_EINVAL, "oww_push_vad: null argument");
    if (h->vad) return fail(OWW_ESTATE, "oww_push_vad: this handle computes its own voice-activity scores (oww_load_vad)");
    HIPCHK(hipSetDevice(h->cfg.device));
    const float* src = vad_scores;
    if (!on_device) {
        HIPCHK(copy_async(h->d_vadin, vad_scores, (size_t)h->S * sizeof(float), hipMemcpyHostToDevice, h->stream));
        src = h->d_vadin;
    }
    hipLaunchKernelGGL(push_vad_kernel, dim3((h->S + 255) / 256), dim3(256), 0, h->stream, h->d_vadring, h->d_nvad, src, h->S);
    HIPCHK(hipGetLastError());
    if (!on_device) HIPCHK(hipStreamSynchronize(h->stream));          // the caller's buffer may be reused at once
    return OWW_OK;
    OWW_GUARD_END
}

int oww_get_vad(oww_ctx* h, float* out) {
    OWW_GUARD_BEGIN
    if (!h || !h->committed) return fail(OWW_ESTATE, "oww_get_vad: handle not committed");
    if (!h->vad) return fail(OWW_ESTATE, "oww_get_vad: no voice-activity network loaded (oww_load_vad)");
    if (!out) return fail(OWW_EINVAL, "oww_get_vad: null argument");
    HIPCHK(hipSetDevice(h->cfg.device));
    HIPCHK(copy_async(out, h->d_vadlast, (size_t)h->S * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return OWW_OK;
    OWW_GUARD_END
}

int oww_reset_vad(oww_ctx* h, const int32_t* stream_ids, int32_t n) {
    OWW_GUARD_BEGIN
    if (!h || !h->committed) return fail(OWW_ESTATE, "oww_reset_vad: handle not committed");
    HIPCHK(hipSetDevice(h->cfg.device));
    const int* d_ids = nullptr;
    int count = h->S;
    if (stream_ids) {
        if (n < 1) return OWW_OK;
        for (int i = 0; i < n; ++i)
            if (stream_ids[i] < 0 || stream_ids[i] >= h->S) return fail(OWW_EINVAL, "oww_reset_vad: stream id %d out of range", stream_ids[i]);
        if (int rc = upload_ids(h, stream_ids, n)) return rc;
        d_ids = h->d_ids; count = n;
    }
    if (h->vad) {
        hipLaunchKernelGGL(owv::vad_reset_kernel, dim3(count), dim3(64), 0, h->stream, h->d_vadhc, h->d_vadring, h->d_nvad, h->d_vadlast, d_ids, count);
    } else {
        hipLaunchKernelGGL(vad_ring_reset_kernel, dim3((count + 255) / 256), dim3(256), 0, h->stream, h->d_vadring, h->d_nvad, d_ids, count);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    return OWW_OK;
    OWW_GUARD_END
}

int oww_sync(oww_ctx* h) {
    OWW_GUARD_BEGIN
    if (!h) return fail(OWW_EINVAL, "null handle");
    HIPCHK(hipSetDevice(h->cfg.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    return range_check(h, "oww_sync");
    OWW_GUARD_END
}

int oww_range_status(oww_ctx* h, int clear) {
    OWW_GUARD_BEGIN
    if (!h || !h->committed) return fail(OWW_ESTATE, "oww_range_status: handle not committed");
    HIPCHK(hipSetDevice(h->cfg.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const int rc = range_check(h, "oww_range_status");
    if (clear && h->h_range) { volatile int* f = (volatile int*)h->h_range; f[1] = -1; f[0] = 0; }     // the position goes with the flag
    return rc;
    OWW_GUARD_END
}

int oww_range_where(oww_ctx* h, int32_t* first_stream, int32_t* n_streams) {
    OWW_GUARD_BEGIN
    if (!h || !h->committed || !first_stream || !n_streams) return fail(OWW_EINVAL, "oww_range_where: bad argument");
    HIPCHK(hipSetDevice(h->cfg.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const volatile int* f = (const volatile int*)h->h_range;
    *first_stream = -1; *n_streams = 0;
    if (f && f[0]) {
        const int packed = f[1];                            // first << 6 | count, written by one wave in one store (owwhip_hx.h)
        if (packed >= 0) {
            const int first = (int)((unsigned)packed >> 6), cnt = packed & 63;
            if (first < h->S && cnt > 0) { *first_stream = first; *n_streams = std::min(cnt, h->S - first); }
        }
    }
    return OWW_OK;
    OWW_GUARD_END
}

const float* oww_scores_dev(const oww_ctx* h) { return h ? h->d_scores : nullptr; }

int oww_resample(oww_ctx* h, const int16_t* in, int in_on_device, int32_t n_in, int32_t p, int32_t q, const float* taps, int32_t n_taps,
                 int16_t* out, int out_on_device, int32_t n_out) {
    OWW_GUARD_BEGIN
    if (!h || !h->committed) return fail(OWW_ESTATE, "oww_resample: handle not committed");
    if (!in) return fail(OWW_EINVAL, "oww_resample: null argument: in");
    if (!taps) return fail(OWW_EINVAL, "oww_resample: null argument: taps");
    if (!out) return fail(OWW_EINVAL, "oww_resample: null argument: out");
    if (n_in < 1 || p < 1 || q < 1 || n_taps < 2 || (n_taps & 1) || n_taps > 4096 || q > 65536)
        return fail(OWW_EINVAL, "oww_resample: bad argument (n_in=%d p=%d q=%d n_taps=%d)", n_in, p, q, n_taps);
    if (n_out != (int32_t)(((long long)n_in * q) / p) || n_out < 1)
        return fail(OWW_EINVAL, "oww_resample: n_out must be n_in * q / p = %lld, got %d", ((long long)n_in * q) / p, n_out);
    HIPCHK(hipSetDevice(h->cfg.device));
    const int ntp = (n_taps + 3) / 4 * 4;
    // outputs per workgroup: as many as a 48 KB input span allows, at most a chunk's worth (the filter bank is staged once per workgroup)
    int opb = RS_NT * 5;
    auto span_of = [&](int o) { return (int)(((long long)(o - 1) * p) / q) + 1 + n_taps + 4; };   // (+ 4: the zero-padded taps read 3 words on)
    while (opb > RS_NT && (size_t)span_of(opb) * sizeof(float) > 48 * 1024) opb -= RS_NT;
    opb = std::min(opb, (n_out + RS_NT - 1) / RS_NT * RS_NT);
    const int span = span_of(opb);
    const size_t lds_x = (size_t)((span + 3) / 4 * 4) * sizeof(float), lds_t = (size_t)q * ntp * sizeof(float);
    if (lds_x > 96 * 1024) return fail(OWW_EINVAL, "oww_resample: input rate too high for the staging buffer (p / q = %d / %d)", p, q);
    const int taps_in_lds = lds_x + lds_t <= 150 * 1024;
    const size_t lds = lds_x + (taps_in_lds ? lds_t : 0);
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(resample_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    const size_t b_taps = ((size_t)q * ntp * sizeof(float) + 255) / 256 * 256;
    const size_t b_in = in_on_device ? 0 : ((size_t)h->S * n_in * sizeof(int16_t) + 255) / 256 * 256;
    const size_t b_out = out_on_device ? 0 : (size_t)h->S * n_out * sizeof(int16_t);
    if (grow(h, h->d_rs, b_taps + b_in + b_out) != hipSuccess) return fail(OWW_ENOMEM, "oww_resample: out of device memory");
    char* base = h->d_rs;
    // (stream-ordered upload from a buffer that lives in the handle: an earlier oww_resample may still be reading the old bank)
    HIPCHK(hipStreamSynchronize(h->stream));
    h->rs_taps.clear();
    owi::bank_pad(taps, q, n_taps, h->rs_taps);
    HIPCHK(copy_async(base, h->rs_taps.data(), h->rs_taps.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
    ResampleParams a{};
    a.taps = (const float*)base; a.n_in = n_in; a.n_out = n_out; a.p = p; a.q = q; a.n_taps = n_taps; a.ntp = ntp; a.S = h->S;
    a.span = span; a.taps_in_lds = taps_in_lds; a.opb = opb;
    a.in = in;
    if (!in_on_device) {
        HIPCHK(copy_async(base + b_taps, in, (size_t)h->S * n_in * sizeof(int16_t), hipMemcpyHostToDevice, h->stream));
        a.in = (const int16_t*)(base + b_taps);
    }
    a.out = out_on_device ? out : (int16_t*)(base + b_taps + b_in);
    hipLaunchKernelGGL(resample_kernel, dim3((n_out + opb - 1) / opb, h->S), dim3(RS_NT), lds, h->stream, a);
    HIPCHK(hipGetLastError());
    if (!out_on_device) {
        HIPCHK(copy_async(out, a.out, (size_t)h->S * n_out * sizeof(int16_t), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    return OWW_OK;
    OWW_GUARD_END
}

// ---- stateful stream ingest, both forms (header: oww_ingest_configure / oww_ingest / oww_step_ingest and oww_ingest_configure_classes /
//      oww_ingest_assign / oww_ingest_mixed / oww_step_ingest_mixed / oww_submit_ingest_mixed).  Every check and all arithmetic is in
//      owwhip_ingest.h; here are the buffers and one of each step: ingest_install behind the two configure entries, ingest_message
//      behind the two ingest entries, step_behind_ingest behind the two step entries.  The launch (launch_ingest, above submit_impl)
//      is where the forms part: ingest_kernel<ENC> for a single-format handle, ingest_mixed_kernel for classes (owwhip_kernels.h) ----

// the handle takes `tab`: the single form's one row, or (mixed) the class table, which goes to the device with a class id per stream
static int ingest_install(oww_ctx* h, const char* fn, owi::Table&& tab, bool mixed) {
    oww_ctx::Ingest& ing = h->ing;
    HIPCHK(hipSetDevice(h->cfg.device));
    HIPCHK(hipStreamSynchronize(h->stream));               // an earlier ingest may still read the old banks and histories
    auto drop = [&] { ing.d_taps.reset(); ing.d_hist.reset(); ing.d_table.reset(); ing.d_cls.reset(); };
    drop();
    ing.ready = false; ing.mixed = false; ing.tab = owi::Table();
    h->d_st_flat.reset(); h->st_ready = false;               // the record layout gains, loses or resizes its ingest sections: rebuilt on demand
    const int Hpad = tab.Hpad_max;
    // (a single form that only decodes has no bank; the table's one placeholder float is there for the class kernel's pointer)
    const size_t n_bank = mixed ? tab.banks.size() : (size_t)tab.dev[0].q * tab.dev[0].ntp, n_hist = (size_t)h->S * Hpad;
    if ((n_bank && ing.d_taps.alloc(n_bank)) || (n_hist && ing.d_hist.alloc(n_hist)) ||
        (mixed && (ing.d_table.alloc(tab.dev.size()) || ing.d_cls.alloc(h->S)))) {
        drop();
        return fail(OWW_ENOMEM, "%s: out of device memory for %d streams x %d history samples and %zu bank floats", fn, h->S, Hpad, n_bank);
    }
    if (n_bank) HIPCHK(copy_sync(ing.d_taps, tab.banks.data(), n_bank * sizeof(float), hipMemcpyHostToDevice));
    if (mixed) {
        HIPCHK(copy_sync(ing.d_table, tab.dev.data(), tab.dev.size() * sizeof(owi::ClassDev), hipMemcpyHostToDevice));
        HIPCHK(hipMemsetAsync(ing.d_cls, 0, (size_t)h->S * sizeof(uint32_t), h->stream));
    }
    if (n_hist) HIPCHK(hipMemsetAsync(ing.d_hist, 0, n_hist * sizeof(int16_t), h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (!ing.d_out) {
        if (ing.d_out.alloc((size_t)h->S * OWW_CHUNK)) return fail(OWW_ENOMEM, "%s: out of device memory", fn);
        HIPCHK(hipMemset(ing.d_out, 0, ing.d_out.capacity() * sizeof(int16_t)));
    }
    ing.tab = std::move(tab);
    ing.mixed = mixed; ing.ready = true;
    return OWW_OK;
}

int oww_ingest_configure(oww_ctx* h, int32_t encoding, int32_t p, int32_t q, const float* taps, int32_t n_taps) {
    OWW_GUARD_BEGIN
    if (!h || !h->committed) return fail(OWW_ESTATE, "oww_ingest_configure: handle not committed");
    const oww_ingest_class one{encoding, p, q, n_taps, taps};
    owi::Table tab;
    if (int rc = owi::table_build("oww_ingest_configure", 1, &one, tab, false)) return rc;
    return ingest_install(h, "oww_ingest_configure", std::move(tab), false);
    OWW_GUARD_END
}

int oww_ingest_configure_classes(oww_ctx* h, int32_t n_classes, const oww_ingest_class* classes) {
    OWW_GUARD_BEGIN
    if (!h || !h->committed) return fail(OWW_ESTATE, "oww_ingest_configure_classes: handle not committed");
    owi::Table tab;
    if (int rc = owi::table_build("oww_ingest_configure_classes", n_classes, classes, tab)) return rc;
    return ingest_install(h, "oww_ingest_configure_classes", std::move(tab), true);
    OWW_GUARD_END
}

const int16_t* oww_ingest_dev(const oww_ctx* h) { return h ? h->ing.d_out : nullptr; }

// the handle is configured, and in the form the entry `fn` serves
static int ingest_ready(const oww_ctx* h, const char* fn, bool mixed) {
    if (!h || !h->committed) return fail(OWW_ESTATE, "%s: handle not committed", fn);
    if (!h->ing.ready) return fail(OWW_ESTATE, "%s: ingest is not configured (%s)", fn, mixed ? "oww_ingest_configure_classes" : "oww_ingest_configure");
    if (mixed && !h->ing.mixed) return fail(OWW_ESTATE, "%s: the handle is configured with oww_ingest_configure, not with ingest classes", fn);
    if (!mixed && h->ing.mixed) return fail(OWW_ESTATE, "%s: the handle is configured with ingest classes: use the _mixed entry", fn);
    return 0;
}

int oww_ingest_assign(oww_ctx* h, const int32_t* stream_ids, int32_t n, const uint8_t* class_ids) {
    OWW_GUARD_BEGIN
    if (int rc = ingest_ready(h, "oww_ingest_assign", true)) return rc;
    if (int rc = owi::assign_check("oww_ingest_assign", h->ing.tab, h->S, stream_ids, n, class_ids)) return rc;
    if (n < 1) return OWW_OK;
    HIPCHK(hipSetDevice(h->cfg.device));
    std::vector<int> cls(class_ids, class_ids + n);
    if (int rc = upload_ids(h, stream_ids, n)) return rc;
    HIPCHK(grow(h, h->ing.d_newcls, (size_t)n));
    HIPCHK(copy_async(h->ing.d_newcls, cls.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(ingest_assign_kernel, dim3(n), dim3(64), 0, h->stream, h->ing.d_hist, h->ing.tab.Hpad_max, h->ing.d_cls, h->d_ids, h->ing.d_newcls, n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));     // host lists may be reused by the caller
    return OWW_OK;
    OWW_GUARD_END
}

// A checked message goes through ingest: `in` is [S][row_bytes] (single form: a row is the message itself), `g` its geometry.  Host
// input and a host mask are staged on the device, a host or absent `out` is served through the 16 kHz staging buffer.
static int ingest_message(oww_ctx* h, const char* fn, const void* in, int in_on_device, long long row_bytes, int n_out, const uint8_t* stream_on,
                          int stream_on_on_device, int16_t* out, int out_on_device, const owi::Geometry& g) {
    oww_ctx::Ingest& ing = h->ing;
    HIPCHK(hipSetDevice(h->cfg.device));
    const size_t in_bytes = (size_t)h->S * (size_t)row_bytes;
    const void* d_in = in;
    if (!in_on_device) {
        if (grow(h, ing.d_in, in_bytes) != hipSuccess) return fail(OWW_ENOMEM, "%s: out of device memory for %zu bytes", fn, in_bytes);
        HIPCHK(copy_async(ing.d_in, in, in_bytes, hipMemcpyHostToDevice, h->stream));
        d_in = ing.d_in;
    }
    const uint8_t* d_on = stream_on;
    if (stream_on && !stream_on_on_device) {
        if (!ing.d_on) HIPCHK(herr(ing.d_on.alloc(h->S)));
        HIPCHK(copy_async(ing.d_on, stream_on, h->S, hipMemcpyHostToDevice, h->stream));
        d_on = ing.d_on;
    }
    const bool to_staging = !out || !out_on_device;
    if (to_staging) {
        const size_t need = (size_t)h->S * n_out;
        if (need > ing.d_out.capacity()) {                   // (a grown staging buffer starts zeroed, like the first)
            if (grow(h, ing.d_out, need) != hipSuccess) return fail(OWW_ENOMEM, "%s: out of device memory for %zu bytes", fn, need * sizeof(int16_t));
            HIPCHK(hipMemset(ing.d_out, 0, need * sizeof(int16_t)));
        }
    }
    if (int rc = launch_ingest(h, d_in, row_bytes, n_out, d_on, to_staging ? (int16_t*)ing.d_out : out, g)) return rc;
    if (out && !out_on_device) {
        const size_t row = (size_t)n_out * sizeof(int16_t);
        if (!stream_on) {
            HIPCHK(copy_async(out, ing.d_out, (size_t)h->S * row, hipMemcpyDeviceToHost, h->stream));
        } else {                                             // only the rows of the streams that took part reach the caller's buffer, run by run
            std::vector<uint8_t> on(h->S);
            if (stream_on_on_device) HIPCHK(hipMemcpy(on.data(), stream_on, h->S, hipMemcpyDeviceToHost)); else memcpy(on.data(), stream_on, h->S);
            for (int s = 0; s < h->S;) {
                if (!on[s]) { ++s; continue; }
                int e = s;
                while (e < h->S && on[e]) ++e;
                HIPCHK(copy_async(out + (size_t)s * n_out, ing.d_out + (size_t)s * n_out, (size_t)(e - s) * row, hipMemcpyDeviceToHost, h->stream));
                s = e;
            }
        }
    }
    if (!in_on_device || (stream_on && !stream_on_on_device) || (out && !out_on_device)) HIPCHK(hipStreamSynchronize(h->stream));   // host buffers are the caller's again
    return OWW_OK;
}

// A checked message goes through ingest and the step behind it, which reads the staging buffer.  `n_out_is` words the single form's
// message ("n_in * q / p = "); every refusal comes before any history moves.
static int step_behind_ingest(oww_ctx* h, const char* fn, const char* n_out_is, const void* in, int in_on_device, long long row_bytes, long long n_out,
                              const uint8_t* stream_on, int stream_on_on_device, float* scores, int scores_on_device, const owi::Geometry& g) {
    if (n_out < OWW_CHUNK || n_out % OWW_CHUNK) return fail(OWW_EINVAL, "%s: n_out = %s%lld must be a positive multiple of %d", fn, n_out_is, n_out, OWW_CHUNK);
    const int n_chunks = (int)(n_out / OWW_CHUNK);
    if (stream_on && n_chunks != 1) return fail(OWW_EINVAL, "%s: a masked step takes one chunk, n_out = %lld", fn, n_out);
    if (stream_on && !h->rr) return fail(OWW_EINVAL, "%s: a masked step needs the register-resident kernel families (use_mfma = 3 or 1)", fn);
    if (n_chunks > OWW_MAX_CALL_CHUNKS) return fail(OWW_EINVAL, "%s: n_chunks=%d outside [1,%d]", fn, n_chunks, OWW_MAX_CALL_CHUNKS);
    if (int rc = range_check(h, fn)) return rc;
    if (int rc = ingest_message(h, fn, in, in_on_device, row_bytes, (int)n_out, stream_on, stream_on_on_device, nullptr, 1, g)) return rc;
    if (stream_on) return oww_step_masked(h, h->ing.d_out, 1, stream_on, stream_on_on_device, scores, scores_on_device);
    return oww_step(h, h->ing.d_out, 1, n_chunks, scores, scores_on_device);
}

int oww_ingest(oww_ctx* h, const void* in, int in_on_device, int32_t n_in, const uint8_t* stream_on, int stream_on_on_device,
               int16_t* out, int out_on_device) {
    OWW_GUARD_BEGIN
    if (int rc = ingest_ready(h, "oww_ingest", false)) return rc;
    long long n_out = 0;
    owi::Geometry g;
    if (int rc = owi::single_check("oww_ingest", h->ing.tab, in, n_in, n_out, g)) return rc;
    return ingest_message(h, "oww_ingest", in, in_on_device, g.min_row_bytes, (int)n_out, stream_on, stream_on_on_device, out, out_on_device, g);
    OWW_GUARD_END
}

int oww_step_ingest(oww_ctx* h, const void* in, int in_on_device, int32_t n_in, const uint8_t* stream_on, int stream_on_on_device,
                    float* scores, int scores_on_device) {
    OWW_GUARD_BEGIN
    if (int rc = ingest_ready(h, "oww_step_ingest", false)) return rc;
    long long n_out = 0;
    owi::Geometry g;
    if (int rc = owi::single_check("oww_step_ingest", h->ing.tab, in, n_in, n_out, g)) return rc;
    return step_behind_ingest(h, "oww_step_ingest", "n_in * q / p = ", in, in_on_device, g.min_row_bytes, n_out, stream_on, stream_on_on_device, scores,
                              scores_on_device, g);
    OWW_GUARD_END
}

int oww_ingest_mixed(oww_ctx* h, const void* in, int in_on_device, int64_t row_bytes, int32_t n_out, const uint8_t* stream_on,
                     int stream_on_on_device, int16_t* out, int out_on_device) {
    OWW_GUARD_BEGIN
    if (int rc = ingest_ready(h, "oww_ingest_mixed", true)) return rc;
    owi::Geometry g;
    if (int rc = owi::mixed_check("oww_ingest_mixed", h->ing.tab, in, row_bytes, n_out, g)) return rc;
    return ingest_message(h, "oww_ingest_mixed", in, in_on_device, row_bytes, n_out, stream_on, stream_on_on_device, out, out_on_device, g);
    OWW_GUARD_END
}

int oww_step_ingest_mixed(oww_ctx* h, const void* in, int in_on_device, int64_t row_bytes, int32_t n_out, const uint8_t* stream_on,
                          int stream_on_on_device, float* scores, int scores_on_device) {
    OWW_GUARD_BEGIN
    if (int rc = ingest_ready(h, "oww_step_ingest_mixed", true)) return rc;
    owi::Geometry g;
    if (int rc = owi::mixed_check("oww_step_ingest_mixed", h->ing.tab, in, row_bytes, n_out, g)) return rc;
    return step_behind_ingest(h, "oww_step_ingest_mixed", "", in, in_on_device, row_bytes, n_out, stream_on, stream_on_on_device, scores, scores_on_device, g);
    OWW_GUARD_END
}

int oww_submit_ingest_mixed(oww_ctx* h, const void* in_host, int64_t row_bytes, const uint8_t* stream_on) {
    OWW_GUARD_BEGIN
    if (int rc = ingest_ready(h, "oww_submit_ingest_mixed", true)) return rc;
    owi::Geometry g;
    if (int rc = owi::mixed_check("oww_submit_ingest_mixed", h->ing.tab, in_host, row_bytes, OWW_CHUNK, g)) return rc;
    if (stream_on && !h->rr)
        return fail(OWW_EINVAL, "oww_submit_ingest_mixed: a masked step needs the register-resident kernel families (use_mfma = 3 or 1; see oww_step_masked)");
    return submit_impl(h, SubmitSource{nullptr, 1, in_host, row_bytes, g}, stream_on);
    OWW_GUARD_END
}

int oww_get_raw(oww_ctx* h, float* out) {
    OWW_GUARD_BEGIN
    if (!h || !h->committed) return fail(OWW_ESTATE, "oww_get_raw: handle not committed");
    if (!out) return fail(OWW_EINVAL, "oww_get_raw: null argument");
    HIPCHK(hipSetDevice(h->cfg.device));
    const size_t nb = (size_t)h->S * h->NL * sizeof(float);
    if (nb) HIPCHK(copy_async(out, h->d_raw, nb, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return OWW_OK;
    OWW_GUARD_END
}

static int mel_impl(oww_ctx* h, const int16_t* pcm, int32_t B, int32_t n, float* out_db, bool per_clip) {
    if (!h || !h->committed) return fail(OWW_ESTATE, "oww_mel: handle not committed");
    if (!pcm || !out_db || B < 1 || n < 512) return fail(OWW_EINVAL, "oww_mel: bad argument (B=%d n=%d)", B, n);
    HIPCHK(hipSetDevice(h->cfg.device));
    const int F = (n - 512) / 160 + 1;
    DevBuf<int16_t> d_in; DevBuf<float> d_out, d_max;
    if (d_in.alloc((size_t)B * n) || d_out.alloc((size_t)B * F * 32) || d_max.alloc(B)) return fail(OWW_ENOMEM, "oww_mel: out of device memory");
    if (copy_async(d_in, pcm, (size_t)B * n * sizeof(int16_t), hipMemcpyHostToDevice, h->stream) != hipSuccess) return drained(h, fail(OWW_EHIP, "oww_mel: H2D failed"));
    if (int rc = launch_mel(h, StepArgs{}, d_in, B, n, F, 0, d_out, d_max)) return drained(h, rc);
    const size_t tot = (size_t)B * F * 32;
    if (per_clip) {
        hipLaunchKernelGGL(clamp_db_rows_kernel, dim3((F * 32 + 255) / 256, B), dim3(256), 0, h->stream, d_out, F * 32, d_max);
    } else {
        std::vector<float> mx(B);
        if (copy_async(mx.data(), d_max, B * sizeof(float), hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
            hipStreamSynchronize(h->stream) != hipSuccess) return drained(h, fail(OWW_EHIP, "oww_mel: D2H failed"));
        float gmax = -INFINITY;                       // one clamp floor for the whole call (ipynb cell 15: log_spec.max())
        for (float v : mx) gmax = std::max(gmax, v);
        hipLaunchKernelGGL(clamp_db_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, h->stream, d_out, tot, gmax - 80.0f);
    }
    if (copy_async(out_db, d_out, tot * sizeof(float), hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
        hipStreamSynchronize(h->stream) != hipSuccess) return drained(h, fail(OWW_EHIP, "oww_mel: D2H failed"));
    return 0;                                         // (synchronised: the buffers are idle when they go)
}

int oww_mel(oww_ctx* h, const int16_t* pcm, int32_t B, int32_t n, float* out_db) { OWW_GUARD_BEGIN return mel_impl(h, pcm, B, n, out_db, false); OWW_GUARD_END }
int oww_mel_clips(oww_ctx* h, const int16_t* pcm, int32_t B, int32_t n, float* out_db) { OWW_GUARD_BEGIN return mel_impl(h, pcm, B, n, out_db, true); OWW_GUARD_END }

int oww_embed(oww_ctx* h, const float* mel_rows, int32_t B, int32_t rows, float* out) {
    OWW_GUARD_BEGIN
    if (!h || !h->committed) return fail(OWW_ESTATE, "oww_embed: handle not committed");
    if (!mel_rows || !out || B < 1 || B > h->Spad || rows < 76 || (rows - 76) % 8) return fail(OWW_EINVAL, "oww_embed: bad argument (B=%d rows=%d, need B<=%d)", B, rows, h->Spad);
    HIPCHK(hipSetDevice(h->cfg.device));
    const int n_out = (rows - 76) / 8 + 1;
    const int n_steps = (rows + 4) / 8;                 // 4 lead-in rows + rows, 8 per step
    std::vector<float> slab((size_t)B * 256), emb((size_t)B * 96);
    const StepArgs a = step_args(h);
    if (int rc = park_state(h, B, true)) return rc;
    int rc_all = 0;
    for (int it = 0; it < n_steps && !rc_all; ++it) {
        for (int b = 0; b < B; ++b)
            for (int r = 0; r < 8; ++r) {
                const int src = it * 8 + r - 4;
                float* d = &slab[((size_t)b * 8 + r) * 32];
                if (src < 0) memset(d, 0, 32 * sizeof(float));
                else memcpy(d, mel_rows + ((size_t)b * rows + src) * 32, 32 * sizeof(float));
            }
        if (copy_async(h->d_mel, slab.data(), slab.size() * sizeof(float), hipMemcpyHostToDevice, h->stream) != hipSuccess) { rc_all = fail(OWW_EHIP, "oww_embed: H2D failed"); break; }
        if ((rc_all = run_cnn(h, a, B, 256, 0))) break;
        hipLaunchKernelGGL(advance_kernel, dim3((h->Spad + 255) / 256), dim3(256), 0, h->stream, h->d_nfeat, h->Spad, (const uint8_t*)nullptr);
        if (it >= 9 && copy_async(emb.data(), h->d_emb, emb.size() * sizeof(float), hipMemcpyDeviceToHost, h->stream) != hipSuccess) { rc_all = fail(OWW_EHIP, "oww_embed: D2H failed"); break; }
        if (hipStreamSynchronize(h->stream) != hipSuccess) { rc_all = fail(OWW_EHIP, "oww_embed: device error"); break; }   // slab is reused next iteration
        if (it >= 9)
            for (int b = 0; b < B; ++b) memcpy(out + ((size_t)b * n_out + (it - 9)) * 96, &emb[(size_t)b * 96], 96 * sizeof(float));
    }
    const int rc_restore = park_state(h, B, false);
    (void)hipStreamSynchronize(h->stream);
    if (rc_all) return rc_all;
    if (rc_restore) return rc_restore;
    return range_check(h, "oww_embed");
    OWW_GUARD_END
}

int oww_embed_clips(oww_ctx* h, const int16_t* pcm, int32_t pcm_on_device, int32_t B, int32_t n, float* out, int32_t out_on_device) {
    OWW_GUARD_BEGIN
    if (!h || !h->committed) return fail(OWW_ESTATE, "oww_embed_clips: handle not committed");
    if (!pcm || !out || B < 1 || B > h->Spad || n < 512) return fail(OWW_EINVAL, "oww_embed_clips: bad argument (B=%d n=%d, need B<=%d)", B, n, h->Spad);
    const int F = (n - 512) / 160 + 1;
    if (F < 76) return fail(OWW_EINVAL, "oww_embed_clips: %d samples give %d mel frames, one embedding window needs 76", n, F);
    if ((int64_t)F * 32 > INT32_MAX / 2) return fail(OWW_EINVAL, "oww_embed_clips: clip too long");
    HIPCHK(hipSetDevice(h->cfg.device));
    const int n_out = (F - 76) / 8 + 1;
    const int n_steps = 9 + n_out;                      // step it consumes mel rows [8 it - 4, 8 it + 4) of every clip
    const int Bp = std::min(h->Spad, (B + 7) / 8 * 8);   // run_cnn covers whole groups of 8 streams: their (zero) mel rows must exist
    const size_t lead = 4 * 32;                         // four lead-in rows in front of clip 0 (other clips: the previous clip's tail;
                                                        // their content never reaches a returned embedding)
    if (int rc = park_state(h, B, true)) return rc;
    DevBuf<int16_t> d_in; DevBuf<float> d_mel, d_max, d_out;
    // the clips' embeddings; whatever it returns, the parked state goes back and the stream is drained before the buffers above go
    auto run = [&]() -> int {
        if (!pcm_on_device) {
            if (d_in.alloc((size_t)B * n)) return fail(OWW_ENOMEM, "oww_embed_clips: out of device memory");
            if (copy_async(d_in, pcm, (size_t)B * n * sizeof(int16_t), hipMemcpyHostToDevice, h->stream) != hipSuccess) return fail(OWW_EHIP, "oww_embed_clips: H2D failed");
        }
        if (d_mel.alloc(lead + (size_t)Bp * F * 32) || d_max.alloc(B) || (!out_on_device && d_out.alloc((size_t)B * n_out * 96)))
            return fail(OWW_ENOMEM, "oww_embed_clips: out of device memory");
        float* o = out_on_device ? out : d_out.get();
        if (hipMemsetAsync(d_mel, 0, lead * sizeof(float), h->stream) != hipSuccess ||
            (Bp > B && hipMemsetAsync(d_mel + lead + (size_t)B * F * 32, 0, (size_t)(Bp - B) * F * 32 * sizeof(float), h->stream) != hipSuccess)) return fail(OWW_EHIP, "oww_embed_clips: memset failed");
        StepArgs a = step_args(h);
        a.mel = d_mel + lead;
        if (int rc = launch_mel(h, a, pcm_on_device ? pcm : d_in.get(), B, n, F, 0, d_mel + lead, d_max)) return rc;
        hipLaunchKernelGGL(clamp_transform_rows_kernel, dim3((F * 32 + 255) / 256, B), dim3(256), 0, h->stream, d_mel + lead, F * 32, d_max);
        for (int it = 0; it < n_steps; ++it) {
            if (int rc = run_cnn(h, a, B, F * 32, (it * 8 - 4) * 32)) return rc;
            hipLaunchKernelGGL(advance_kernel, dim3((h->Spad + 255) / 256), dim3(256), 0, h->stream, h->d_nfeat, h->Spad, (const uint8_t*)nullptr);
            if (it >= 9 && hipMemcpy2DAsync(o + (size_t)(it - 9) * 96, (size_t)n_out * 96 * sizeof(float), h->d_emb, 96 * sizeof(float),
                                            96 * sizeof(float), B, hipMemcpyDeviceToDevice, h->stream) != hipSuccess)
                return fail(OWW_EHIP, "oww_embed_clips: gather failed");
        }
        if (!out_on_device && copy_async(out, d_out, (size_t)B * n_out * 96 * sizeof(float), hipMemcpyDeviceToHost, h->stream) != hipSuccess) return fail(OWW_EHIP, "oww_embed_clips: D2H failed");
        if (hipStreamSynchronize(h->stream) != hipSuccess) return fail(OWW_EHIP, "oww_embed_clips: device error: %s", hipGetErrorString(hipGetLastError()));
        return 0;
    };
    const int rc = run();
    const int rc_restore = park_state(h, B, false);
    (void)hipStreamSynchronize(h->stream);
    if (rc) return rc;
    if (rc_restore) return rc_restore;
    return range_check(h, "oww_embed_clips");
    OWW_GUARD_END
}

int oww_head(oww_ctx* h, int32_t head, const float* features, int32_t B, float* out) {
    OWW_GUARD_BEGIN
    if (!h || !h->committed) return fail(OWW_ESTATE, "oww_head: handle not committed");
    if (head < 0 || head >= (int)h->heads.size() || !features || !out || B < 1) return fail(OWW_EINVAL, "oww_head: bad argument");
    HIPCHK(hipSetDevice(h->cfg.device));
    const HeadHost& hh = h->heads[head];
    const size_t nf = (size_t)B * hh.T * 96;
    DevBuf<float> d_f, d_raw;
    if (d_f.alloc(nf) || d_raw.alloc((size_t)B * h->NL)) return fail(OWW_ENOMEM, "oww_head: out of device memory");
    if (copy_async(d_f, features, nf * sizeof(float), hipMemcpyHostToDevice, h->stream) != hipSuccess) return drained(h, fail(OWW_EHIP, "oww_head: H2D failed"));
    if (hipMemsetAsync(d_raw, 0, (size_t)B * h->NL * sizeof(float), h->stream) != hipSuccess) return drained(h, fail(OWW_EHIP, "oww_head: memset failed"));
    if (int rc = run_heads(h, step_args(h), B, false, d_f, head, d_raw, 0)) return drained(h, rc);
    std::vector<float> raw((size_t)B * h->NL);
    if (copy_async(raw.data(), d_raw, raw.size() * sizeof(float), hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
        hipStreamSynchronize(h->stream) != hipSuccess) return drained(h, fail(OWW_EHIP, "oww_head: D2H failed"));
    for (int b = 0; b < B; ++b)
        for (int o = 0; o < hh.n_out; ++o) out[(size_t)b * hh.n_out + o] = raw[(size_t)b * h->NL + hh.out_col + o];
    return range_check(h, "oww_head");
    OWW_GUARD_END
}

// ---- dense scoring: oww_score_shape, oww_score_features, oww_score_clips (helpers: score_device above)
int oww_score_shape(oww_ctx* h, int32_t n_rows, int32_t* n_win, int32_t* t_max) {
    OWW_GUARD_BEGIN
    if (int rc = owd::ready_check("oww_score_shape", h != nullptr, h && h->committed, h ? (int)h->heads.size() : 0)) return rc;
    const int tm = dense_t_max(h);
    if (int rc = owd::shape_check("oww_score_shape", n_rows, tm)) return rc;
    if (n_win) *n_win = (int32_t)owd::n_win(n_rows, tm);
    if (t_max) *t_max = tm;
    return 0;
    OWW_GUARD_END
}

int oww_score_features(oww_ctx* h, const float* feats, int feats_on_device, int32_t B, int32_t n_rows, float* out, int out_on_device) {
    OWW_GUARD_BEGIN
    const char* fn = "oww_score_features";
    if (int rc = owd::ready_check(fn, h != nullptr, h && h->committed, h ? (int)h->heads.size() : 0)) return rc;
    const int t_max = dense_t_max(h);
    if (int rc = owd::features_check(fn, feats, feats_on_device, B, n_rows, t_max, h->NL, out, out_on_device)) return rc;
    HIPCHK(hipSetDevice(h->cfg.device));
    DenseIO io{h, fn};
    if (int rc = io.open(feats, feats_on_device, owd::feats_bytes(B, n_rows), out, out_on_device, owd::out_bytes(B, owd::n_win(n_rows, t_max), h->NL))) return rc;
    if (int rc = score_device(h, fn, io.feats, B, n_rows, io.out)) return drained(h, rc);
    return io.finish();
    OWW_GUARD_END
}

int oww_score_clips(oww_ctx* h, const int16_t* pcm, int pcm_on_device, int32_t B, int32_t n, float* out, int out_on_device, float* emb_out,
                    int emb_on_device) {
    OWW_GUARD_BEGIN
    const char* fn = "oww_score_clips";
    if (int rc = owd::ready_check(fn, h != nullptr, h && h->committed, h ? (int)h->heads.size() : 0)) return rc;
    const int t_max = dense_t_max(h);
    if (int rc = owd::clips_check(fn, pcm, B, n, h->Spad, t_max, h->NL, out)) return rc;
    HIPCHK(hipSetDevice(h->cfg.device));
    const int n_rows = (int)owd::clip_rows(n);
    const uint64_t fb = owd::feats_bytes(B, n_rows);
    DenseIO io{h, fn};
    if (int rc = io.open(nullptr, 0, fb, out, out_on_device, owd::out_bytes(B, owd::n_win(n_rows, t_max), h->NL))) return rc;
    if (int rc = oww_embed_clips(h, pcm, pcm_on_device, B, n, io.d_f, 1)) return rc;   // parks and restores streams [0, B); drained on return
    if (int rc = score_device(h, fn, io.feats, B, n_rows, io.out)) return drained(h, rc);
    if (int rc = io.download()) return rc;
    if (emb_out && copy_async(emb_out, io.d_f, fb, emb_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream) != hipSuccess)
        return drained(h, fail(OWW_EHIP, "%s: embedding copy failed", fn));
    return io.settle();
    OWW_GUARD_END
}

// ---- dense scoring over the head bank: oww_bank_score_shape, oww_bank_score_features, oww_bank_score_stats (bank_score_device above)
int oww_bank_score_shape(oww_ctx* h, const int32_t* bank_ids, int32_t n_ids, int32_t n_rows, int32_t* n_win, int32_t* t_max) {
    OWW_GUARD_BEGIN
    const char* fn = "oww_bank_score_shape";
    if (int rc = owd::bank_ready_check(fn, h != nullptr, h && h->committed, h ? h->bank_K : 0)) return rc;
    int tm = 0;
    if (int rc = owd::bank_ids_check(fn, bank_ids, n_ids, bank_live_T(h).data(), h->bank_cap, &tm)) return rc;
    if (int rc = owd::shape_check(fn, n_rows, tm)) return rc;
    if (n_win) *n_win = (int32_t)owd::n_win(n_rows, tm);
    if (t_max) *t_max = tm;
    return 0;
    OWW_GUARD_END
}

int oww_bank_score_features(oww_ctx* h, const float* feats, int feats_on_device, int32_t B, int32_t n_rows, const int32_t* bank_ids, int32_t n_ids,
                            float* out, int out_on_device) {
    OWW_GUARD_BEGIN
    const char* fn = "oww_bank_score_features";
    if (int rc = owd::bank_ready_check(fn, h != nullptr, h && h->committed, h ? h->bank_K : 0)) return rc;
    int t_max = 0;
    if (int rc = owd::bank_ids_check(fn, bank_ids, n_ids, bank_live_T(h).data(), h->bank_cap, &t_max)) return rc;
    if (int rc = owd::bank_features_check(fn, feats, feats_on_device, B, n_rows, t_max, n_ids, out, out_on_device)) return rc;
    HIPCHK(hipSetDevice(h->cfg.device));
    DenseIO io{h, fn};
    if (int rc = io.open(feats, feats_on_device, owd::feats_bytes(B, n_rows), out, out_on_device, owd::out_bytes(B, owd::n_win(n_rows, t_max), n_ids))) return rc;
    // (drained: bank_score_device returns undrained where its head list could not be allocated or uploaded, with the features in flight)
    if (int rc = bank_score_device(h, fn, io.feats, B, n_rows, bank_ids, n_ids, t_max, io.out, nullptr, nullptr, nullptr, nullptr)) return drained(h, rc);
    return io.finish();
    OWW_GUARD_END
}

int oww_bank_score_stats(oww_ctx* h, const float* feats, int feats_on_device, int32_t B, int32_t n_rows, const int32_t* bank_ids, int32_t n_ids,
                         const float* thresholds, int32_t* count, float* max, int32_t* argmax) {
    OWW_GUARD_BEGIN
    const char* fn = "oww_bank_score_stats";
    if (int rc = owd::bank_ready_check(fn, h != nullptr, h && h->committed, h ? h->bank_K : 0)) return rc;
    int t_max = 0;
    if (int rc = owd::bank_ids_check(fn, bank_ids, n_ids, bank_live_T(h).data(), h->bank_cap, &t_max)) return rc;
    if (int rc = owd::bank_stats_check(fn, feats, feats_on_device, B, n_rows, t_max, n_ids, thresholds, count, max, argmax)) return rc;
    HIPCHK(hipSetDevice(h->cfg.device));
    const uint64_t fb = owd::feats_bytes(B, n_rows);
    const size_t cells = (size_t)B * (size_t)n_ids;
    std::vector<float> thr((size_t)n_ids, 0.5f);                // train.py:100's default
    if (thresholds) thr.assign(thresholds, thresholds + n_ids);
    DenseIO io{h, fn};
    DevBuf<float> d_thr; DevBuf<int> d_count; DevBuf<unsigned long long> d_key;
    if (io.alloc_feats(feats, feats_on_device, fb) || d_thr.alloc((size_t)n_ids) || d_count.alloc(cells) || d_key.alloc(cells))
        return fail(OWW_ENOMEM, "%s: out of device memory (%llu bytes of features, %llu bytes of statistics)", fn, (unsigned long long)fb,
                    (unsigned long long)owd::stats_bytes(B, n_ids));
    if (io.upload(feats, fb) != hipSuccess ||
        copy_async(d_thr, thr.data(), thr.size() * sizeof(float), hipMemcpyHostToDevice, h->stream) != hipSuccess ||
        hipMemsetAsync(d_count, 0, cells * sizeof(int), h->stream) != hipSuccess ||
        hipMemsetAsync(d_key, 0, cells * sizeof(unsigned long long), h->stream) != hipSuccess) return drained(h, fail(OWW_EHIP, "%s: H2D failed", fn));
    if (int rc = bank_score_device(h, fn, io.feats, B, n_rows, bank_ids, n_ids, t_max, nullptr, d_thr, thr.data(), d_count, d_key))
        return drained(h, rc);
    std::vector<unsigned long long> key(cells);
    if (copy_async(count, d_count, cells * sizeof(int), hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
        copy_async(key.data(), d_key, cells * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream) != hipSuccess) return drained(h, fail(OWW_EHIP, "%s: D2H failed", fn));
    if (hipStreamSynchronize(h->stream) != hipSuccess) return fail(OWW_EHIP, "%s: device error: %s", fn, hipGetErrorString(hipGetLastError()));
    for (size_t c = 0; c < cells; ++c) {
        const uint32_t bits = owd::stat_key_bits(key[c]);
        memcpy(&max[c], &bits, sizeof bits);
        argmax[c] = (int32_t)owd::stat_key_window(key[c]);
    }
    if (h->h_range && *(volatile int*)h->h_range)
        return fail(OWW_ERANGE, "%s: an activation left the f16 range of the fp16-split kernels -- the statistics of this call are not defined (a score "
                    "that is no number takes part in neither the count nor the maximum in a defined way); clear with oww_range_status(h, 1)", fn);
    return 0;
    OWW_GUARD_END
}

// ---- ordered hit lists of dense scoring: oww_score_hits_layout, oww_score_hits, oww_score_clip_hits, oww_bank_score_hits
int oww_score_hits_layout(oww_ctx* h, const int32_t* bank_ids, int32_t n_ids, int32_t cap, int64_t* win_offset) {
    OWW_GUARD_BEGIN
    const char* fn = "oww_score_hits_layout";
    std::vector<int> T, head;
    if (bank_ids) {
        if (int rc = owd::bank_ready_check(fn, h != nullptr, h && h->committed, h ? h->bank_K : 0)) return rc;
        int t_max = 0;
        if (int rc = owd::bank_ids_check(fn, bank_ids, n_ids, bank_live_T(h).data(), h->bank_cap, &t_max)) return rc;
        for (int i = 0; i < n_ids; ++i) T.push_back(h->bank[bank_ids[i]].T);
    } else {
        if (int rc = owd::ready_check(fn, h != nullptr, h && h->committed, h ? (int)h->heads.size() : 0)) return rc;
        fixed_columns(h, T, head);
    }
    if (int rc = owdh::layout_check(fn, cap, win_offset)) return rc;
    owdh::win_offsets(T.data(), (int64_t)T.size(), cap, win_offset);
    return 0;
    OWW_GUARD_END
}

int oww_score_hits(oww_ctx* h, const float* feats, int feats_on_device, int32_t B, int32_t n_rows, const float* thresholds, int32_t cap,
                   oww_dense_hit* hits, int32_t* n_stored, int64_t* n_total, float* windows, int windows_on_device) {
    OWW_GUARD_BEGIN
    const char* fn = "oww_score_hits";
    if (int rc = owd::ready_check(fn, h != nullptr, h && h->committed, h ? (int)h->heads.size() : 0)) return rc;
    if (int rc = owdh::features_check(fn, feats, feats_on_device, B, n_rows, dense_t_max(h), h->NL, cap, hits, n_stored, n_total, windows, windows_on_device)) return rc;
    HIPCHK(hipSetDevice(h->cfg.device));
    const uint64_t fb = owd::feats_bytes(B, n_rows);
    DenseIO io{h, fn};
    if (io.alloc_feats(feats, feats_on_device, fb)) return fail(OWW_ENOMEM, "%s: out of device memory (%llu bytes of features)", fn, (unsigned long long)fb);
    if (io.upload(feats, fb) != hipSuccess) return drained(h, fail(OWW_EHIP, "%s: H2D failed", fn));
    return drained(h, score_hits_device(h, fn, io.feats, B, n_rows, thresholds, cap, hits, n_stored, n_total, windows, windows_on_device));
    OWW_GUARD_END
}

int oww_score_clip_hits(oww_ctx* h, const int16_t* pcm, int pcm_on_device, int32_t B, int32_t n, const float* thresholds, int32_t cap,
                        oww_dense_hit* hits, int32_t* n_stored, int64_t* n_total, float* windows, int windows_on_device) {
    OWW_GUARD_BEGIN
    const char* fn = "oww_score_clip_hits";
    if (int rc = owd::ready_check(fn, h != nullptr, h && h->committed, h ? (int)h->heads.size() : 0)) return rc;
    if (int rc = owdh::clips_check(fn, pcm, B, n, h->Spad, dense_t_max(h), h->NL, cap, hits, n_stored, n_total, windows, windows_on_device)) return rc;
    HIPCHK(hipSetDevice(h->cfg.device));
    const int n_rows = (int)owd::clip_rows(n);
    const uint64_t fb = owd::feats_bytes(B, n_rows);
    DevBuf<float> d_emb;            // the embeddings stay here: only hits and their windows go back
    if (d_emb.alloc((size_t)(fb / 4))) return fail(OWW_ENOMEM, "%s: out of device memory (%llu bytes of embeddings)", fn, (unsigned long long)fb);
    if (int rc = oww_embed_clips(h, pcm, pcm_on_device, B, n, d_emb, 1)) return rc;      // parks and restores streams [0, B); drained on return
    return drained(h, score_hits_device(h, fn, d_emb, B, n_rows, thresholds, cap, hits, n_stored, n_total, windows, windows_on_device));
    OWW_GUARD_END
}

int oww_bank_score_hits(oww_ctx* h, const float* feats, int feats_on_device, int32_t B, int32_t n_rows, const int32_t* bank_ids, int32_t n_ids,
                        const float* thresholds, int32_t cap, oww_dense_hit* hits, int32_t* n_stored, int64_t* n_total, float* windows,
                        int windows_on_device) {
    OWW_GUARD_BEGIN
    const char* fn = "oww_bank_score_hits";
    if (int rc = owd::bank_ready_check(fn, h != nullptr, h && h->committed, h ? h->bank_K : 0)) return rc;
    int t_max = 0;
    if (int rc = owd::bank_ids_check(fn, bank_ids, n_ids, bank_live_T(h).data(), h->bank_cap, &t_max)) return rc;
    if (int rc = owdh::features_check(fn, feats, feats_on_device, B, n_rows, t_max, n_ids, cap, hits, n_stored, n_total, windows, windows_on_device)) return rc;
    if (int rc = owdh::bank_thresholds_check(fn, thresholds, n_ids)) return rc;
    HIPCHK(hipSetDevice(h->cfg.device));
    const uint64_t fb = owd::feats_bytes(B, n_rows);
    std::vector<float> thr((size_t)n_ids, 0.5f);                // train.py:100's default
    if (thresholds) thr.assign(thresholds, thresholds + n_ids);
    std::vector<int> T;
    for (int i = 0; i < n_ids; ++i) T.push_back(h->bank[bank_ids[i]].T);
    DenseIO io{h, fn};
    if (io.alloc_feats(feats, feats_on_device, fb)) return fail(OWW_ENOMEM, "%s: out of device memory (%llu bytes of features)", fn, (unsigned long long)fb);
    if (io.upload(feats, fb) != hipSuccess) return drained(h, fail(OWW_EHIP, "%s: H2D failed", fn));
    HitsBuf hb;
    if (int rc = hits_open(h, fn, B, owd::n_win(n_rows, t_max), n_ids, cap, thr, hb)) return drained(h, rc);
    if (int rc = bank_score_device(h, fn, io.feats, B, n_rows, bank_ids, n_ids, t_max, nullptr, hb.d_thr, thr.data(), nullptr, nullptr, &hb.ms)) return drained(h, rc);
    BankRescorer rs(h, fn, bank_ids);
    return drained(h, hits_finish(h, fn, io.feats, B, n_rows, t_max, n_ids, T, hb, rs, hits, n_stored, n_total, windows, windows_on_device));
    OWW_GUARD_END
}

int oww_get_features(oww_ctx* h, int32_t sid, int32_t T, float* out) {
    OWW_GUARD_BEGIN
    if (!h || !h->committed) return fail(OWW_ESTATE, "oww_get_features: handle not committed");
    if (sid < 0 || sid >= h->S || T < 1 || T > h->TR || !out) return fail(OWW_EINVAL, "oww_get_features: bad argument (sid=%d T=%d ring=%d)", sid, T, h->TR);
    HIPCHK(hipSetDevice(h->cfg.device));
    std::vector<float> ring((size_t)h->TR * 96);
    uint32_t cnt = 0;
    HIPCHK(copy_async(ring.data(), h->d_feat + (size_t)sid * h->TR * 96, ring.size() * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(copy_async(&cnt, h->d_nfeat + sid, sizeof cnt, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    // after the step's advance the newest row sits at slot (cnt-1) % TR; oldest-first order of the last T rows
    for (int t = 0; t < T; ++t) {
        const uint32_t slot = (cnt + (uint32_t)(2 * h->TR - T + t)) % (uint32_t)h->TR;
        memcpy(out + (size_t)t * 96, &ring[(size_t)slot * 96], 96 * sizeof(float));
    }
    return OWW_OK;
    OWW_GUARD_END
}

int oww_get_mel(oww_ctx* h, int32_t sid, float* out, int32_t n_rows) {
    OWW_GUARD_BEGIN
    if (!h || !h->committed) return fail(OWW_ESTATE, "oww_get_mel: handle not committed");
    if (h->fuse && h->k_last == 1 && !h->cfg.debug_layers)
        return fail(OWW_ESTATE, "oww_get_mel: with the mel front end fused into stage A the rows of a one-chunk step never reach HBM; "
                    "create the handle with debug_layers = 1 to keep them");
    const int rows_last = 8 * h->k_last;           // the last step wrote [S][8 * n_chunks][32]
    if (sid < 0 || sid >= h->S || !out || n_rows < 1 || n_rows > rows_last)
        return fail(OWW_EINVAL, "oww_get_mel: bad argument (sid=%d n_rows=%d; the last step produced %d rows per stream)", sid, n_rows, rows_last);
    HIPCHK(hipSetDevice(h->cfg.device));
    HIPCHK(copy_async(out, h->d_mel + ((size_t)sid * rows_last + (rows_last - n_rows)) * 32, (size_t)n_rows * 32 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return OWW_OK;
    OWW_GUARD_END
}

int oww_debug_read(oww_ctx* h, int32_t sid, int32_t layer, float* out, int32_t cap) {
    OWW_GUARD_BEGIN
    if (!h || !h->committed || !h->d_dbg) return fail(OWW_ESTATE, "oww_debug_read: needs a committed handle created with debug_layers=1");
    if (sid < 0 || sid >= h->S || layer < 0 || layer > 19 || !out) return fail(OWW_EINVAL, "oww_debug_read: bad argument");
    int off = 0;
    for (int l = 0; l < layer; ++l) off += kLayerOut[l][0] * kLayerOut[l][1] * kLayerOut[l][2];
    const int n = kLayerOut[layer][0] * kLayerOut[layer][1] * kLayerOut[layer][2];
    if (cap < n) return fail(OWW_EINVAL, "oww_debug_read: need room for %d floats", n);
    HIPCHK(hipSetDevice(h->cfg.device));
    HIPCHK(copy_async(out, h->d_dbg + (size_t)sid * DBG_FLOATS + off, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return n;
    OWW_GUARD_END
}

int oww_debug_profile(oww_ctx* h, int64_t* out, int32_t cap) {
    OWW_GUARD_BEGIN
    if (!h || !h->committed || !h->d_prof) return fail(OWW_ESTATE, "oww_debug_profile: set OWW_PROF_BLOCK before creating the handle");
    if (!out || cap < 4 * 256) return fail(OWW_EINVAL, "oww_debug_profile: need room for 1024 values");
    HIPCHK(hipSetDevice(h->cfg.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(copy_sync(out, h->d_prof, (size_t)4 * 256 * sizeof(long long), hipMemcpyDeviceToHost));
    return 4 * 256;
    OWW_GUARD_END
}

int oww_enable_timing(oww_ctx* h, int on) {
    OWW_GUARD_BEGIN
    if (!h) return fail(OWW_EINVAL, "null handle");
    if (!on && h->timing) { if (int rc = flush_events(h)) return rc; }
    h->timing = on != 0;
    return OWW_OK;
    OWW_GUARD_END
}

int oww_kernel_times(oww_ctx* h, double ms[OWW_N_KERNEL_CLASSES], int64_t n[OWW_N_KERNEL_CLASSES]) {
    OWW_GUARD_BEGIN
    if (!h || !ms || !n) return fail(OWW_EINVAL, "null argument");
    HIPCHK(hipSetDevice(h->cfg.device));
    if (int rc = flush_events(h)) return rc;
    for (int i = 0; i < OWW_N_KERNEL_CLASSES; ++i) { ms[i] = h->t_ms[i]; n[i] = h->t_n[i]; h->t_ms[i] = 0; h->t_n[i] = 0; }
    return OWW_OK;
    OWW_GUARD_END
}

int oww_use_graph(oww_ctx* h, int on) {
    OWW_GUARD_BEGIN
    if (!h) return fail(OWW_EINVAL, "null handle");
    h->want_graph = on != 0;
    if (!on && h->graph_exec) { (void)hipGraphExecDestroy(h->graph_exec); h->graph_exec = nullptr; }
    return OWW_OK;
    OWW_GUARD_END
}

// ---- multi-GPU delivery of results over RCCL, without torch.distributed -----------------------------------------------------------
// ---- head bank ------------------------------------------------------------------------------------------------------------------------
int oww_events_configure(oww_ctx* h, int32_t capacity, int32_t feature_rows) {
    OWW_GUARD_BEGIN
    if (!h) return fail(OWW_EINVAL, "oww_events_configure: null handle");
    if (h->committed) return fail(OWW_ESTATE, "oww_events_configure: call before oww_commit");
    if (capacity < 1 || capacity > (1 << 20)) return fail(OWW_EINVAL, "oww_events_configure: capacity = %d outside [1, %d]", capacity, 1 << 20);
    // (the upper limit is the handle's feature ring, which is known once every head is loaded: oww_commit refuses what exceeds it)
    if (feature_rows < 0) return fail(OWW_EINVAL, "oww_events_configure: feature_rows = %d outside [0, the feature ring]", feature_rows);
    h->evt_cap = capacity; h->evt_rows = feature_rows;
    return OWW_OK;
    OWW_GUARD_END
}

int oww_events_set_thresholds(oww_ctx* h, const float* fixed, float bank) {
    OWW_GUARD_BEGIN
    if (!h) return fail(OWW_EINVAL, "oww_events_set_thresholds: null handle");
    if (!h->committed || !events_on(h)) return fail(OWW_ESTATE, "oww_events_set_thresholds: needs oww_events_configure and oww_commit");
    HIPCHK(hipSetDevice(h->cfg.device));
    if (fixed && h->NL > 0) {
        HIPCHK(copy_async(h->d_evt_thr, fixed, (size_t)h->NL * sizeof(float), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));     // the caller's array is free again
    }
    if (bank == bank) h->evt_bank_thr = bank;
    return OWW_OK;
    OWW_GUARD_END
}

// {n_stored, n_total} of the call oww_get_events refers to
static int event_counts(oww_ctx* h, int cnt[2]) {
    cnt[0] = cnt[1] = 0;
    const oww_ctx::EventBuf* b = h->evt_cur;
    if (!b) return 0;
    if (b->h_count) { cnt[0] = b->h_count[0]; cnt[1] = b->h_count[1]; return 0; }
    HIPCHK(copy_async(cnt, b->d_count, 2 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

int oww_get_events(oww_ctx* h, oww_event* out, int32_t cap, int32_t* n_stored, int32_t* n_total) {
    OWW_GUARD_BEGIN
    if (!h) return fail(OWW_EINVAL, "oww_get_events: null handle");
    if (!h->committed || !events_on(h)) return fail(OWW_ESTATE, "oww_get_events: the handle has no events (oww_events_configure before oww_commit)");
    if (cap < 0 || (cap > 0 && !out)) return fail(OWW_EINVAL, "oww_get_events: cap = %d with out = %p", cap, (void*)out);
    HIPCHK(hipSetDevice(h->cfg.device));
    int cnt[2];
    if (int rc = event_counts(h, cnt)) return rc;
    const int n = std::min(std::min(cnt[0], h->evt_cap), (int)cap);
    if (n > 0 && out) {
        const oww_ctx::EventBuf* b = h->evt_cur;
        if (b->h_rec) memcpy(out, b->h_rec, (size_t)n * sizeof(oww_event));
        else {
            HIPCHK(copy_async(out, b->d_rec, (size_t)n * sizeof(oww_event), hipMemcpyDeviceToHost, h->stream));
            HIPCHK(hipStreamSynchronize(h->stream));
        }
    }
    if (n_stored) *n_stored = cnt[0];
    if (n_total) *n_total = cnt[1];
    return OWW_OK;
    OWW_GUARD_END
}

int oww_get_event_features(oww_ctx* h, int32_t first, int32_t n, float* out, int out_on_device) {
    OWW_GUARD_BEGIN
    if (!h) return fail(OWW_EINVAL, "oww_get_event_features: null handle");
    if (!h->committed || !events_on(h)) return fail(OWW_ESTATE, "oww_get_event_features: the handle has no events (oww_events_configure before oww_commit)");
    if (h->evt_rows == 0) return fail(OWW_EINVAL, "oww_get_event_features: the handle keeps no snapshots (feature_rows = 0)");
    HIPCHK(hipSetDevice(h->cfg.device));
    int cnt[2];
    if (int rc = event_counts(h, cnt)) return rc;
    const int stored = std::min(cnt[0], h->evt_cap);
    if (first < 0 || n < 0 || (long long)first + n > stored) return fail(OWW_EINVAL, "oww_get_event_features: events [%d, %d + %d) of %d stored", first, first, n, stored);
    if (n == 0) return OWW_OK;
    if (!out) return fail(OWW_EINVAL, "oww_get_event_features: out is null");
    const size_t per = (size_t)h->evt_rows * OWW_EMB_DIM;
    HIPCHK(copy_async(out, h->evt_cur->d_snap + (size_t)first * per, (size_t)n * per * sizeof(float),
                      out_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return OWW_OK;
    OWW_GUARD_END
}

const oww_event* oww_events_dev(const oww_ctx* h, const int32_t** count_dev) {
    const bool ok = h && h->committed && events_on(h);
    if (count_dev) *count_dev = ok ? h->evt_sync.d_count : nullptr;
    return ok ? h->evt_sync.d_rec : nullptr;
}

const float* oww_event_features_dev(const oww_ctx* h) { return h && h->committed && events_on(h) ? h->evt_sync.d_snap : nullptr; }

int oww_audio_configure(oww_ctx* h, int32_t ring_chunks, int32_t event_chunks) {
    OWW_GUARD_BEGIN
    if (int rc = owa::configure_check(h != nullptr, h && h->committed, ring_chunks, event_chunks)) return rc;
    h->aud_ring = ring_chunks; h->aud_evt = event_chunks;
    return OWW_OK;
    OWW_GUARD_END
}

int oww_get_audio(oww_ctx* h, const int32_t* stream_ids, int32_t n, int32_t n_chunks, int16_t* out, int out_on_device, uint32_t* counts) {
    OWW_GUARD_BEGIN
    if (int rc = owa::ready_check("oww_get_audio", h != nullptr, h && h->committed, h ? h->aud_ring : 0)) return rc;
    if (int rc = owa::get_audio_check(h->S, h->aud_ring, stream_ids, n, n_chunks, out, out_on_device)) return rc;
    if (n == 0) return OWW_OK;
    HIPCHK(hipSetDevice(h->cfg.device));
    const uint64_t nb = owa::gather_bytes(n, n_chunks);
    if (grow(h, h->d_aids, (size_t)n) != hipSuccess || grow(h, h->d_acnt, (size_t)n) != hipSuccess)
        return fail(OWW_ENOMEM, "oww_get_audio: out of device memory for a list of %d streams", n);
    if (!out_on_device && grow(h, h->d_aout, (size_t)(nb / sizeof(int16_t))) != hipSuccess)
        return fail(OWW_ENOMEM, "oww_get_audio: out of device memory for %llu bytes", (unsigned long long)nb);
    HIPCHK(copy_async(h->d_aids, stream_ids, (size_t)n * sizeof(int), hipMemcpyHostToDevice, h->stream));
    owa::GatherParams p{};
    p.ring = h->d_aring; p.counter = h->d_acount; p.ids = h->d_aids; p.out = out_on_device ? out : (int16_t*)h->d_aout; p.counts = h->d_acnt;
    p.S = h->S; p.n_chunks = (uint32_t)n_chunks; p.ring_chunks = (uint32_t)h->aud_ring;
    const int per_launch = std::max(1, (1 << 25) / n_chunks);          // (a launch stays below 2^32 threads: 2^25 waves)
    for (int at = 0; at < n; at += per_launch) {
        const int m = std::min(n - at, per_launch);
        owa::GatherParams q = p;
        q.ids = p.ids + at; q.out = p.out + (size_t)at * n_chunks * OWW_CHUNK; q.counts = p.counts + at;
        hipLaunchKernelGGL(owa::audio_gather_kernel, dim3(m, n_chunks), dim3(64), 0, h->stream, q);
    }
    HIPCHK(hipGetLastError());
    if (!out_on_device) HIPCHK(copy_async(out, h->d_aout, (size_t)nb, hipMemcpyDeviceToHost, h->stream));
    if (counts) HIPCHK(copy_async(counts, h->d_acnt, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));           // behind every queued step; the host list was a copy source, host buffers are complete
    return OWW_OK;
    OWW_GUARD_END
}

int oww_get_event_audio(oww_ctx* h, int32_t first, int32_t n, int16_t* out, int out_on_device) {
    OWW_GUARD_BEGIN
    if (int rc = owa::ready_check("oww_get_event_audio", h != nullptr, h && h->committed, h ? h->aud_ring : 0)) return rc;
    HIPCHK(hipSetDevice(h->cfg.device));
    int cnt[2] = {0, 0};
    if (h->aud_evt > 0) if (int rc = event_counts(h, cnt)) return rc;
    if (int rc = owa::event_audio_check(h->aud_evt, first, n, std::min(cnt[0], h->evt_cap), out, out_on_device)) return rc;
    if (n == 0) return OWW_OK;
    const size_t per = (size_t)h->aud_evt * OWW_CHUNK;
    HIPCHK(copy_async(out, h->evt_cur->d_asnap + (size_t)first * per, (size_t)n * per * sizeof(int16_t),
                      out_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return OWW_OK;
    OWW_GUARD_END
}

const int16_t* oww_event_audio_dev(const oww_ctx* h) { return h && h->committed && h->aud_evt > 0 ? h->evt_sync.d_asnap.get() : nullptr; }

int oww_bank_configure(oww_ctx* h, int32_t slots, int32_t capacity) {
    OWW_GUARD_BEGIN
    if (!h) return fail(OWW_EINVAL, "null handle");
    if (h->committed) return fail(OWW_ESTATE, "oww_bank_configure: call before oww_commit");
    if (!h->hx) return fail(OWW_ESTATE, "oww_bank_configure: the head bank runs on the fp16-split heads kernels (use_mfma = 3) only");
    if (slots < 1 || slots > 8) return fail(OWW_EINVAL, "oww_bank_configure: slots = %d (1..8)", slots);
    if (capacity < 1 || capacity > 65536) return fail(OWW_EINVAL, "oww_bank_configure: capacity = %d (1..65536)", capacity);
    h->bank_K = slots; h->bank_cap = capacity;
    return OWW_OK;
    OWW_GUARD_END
}

int oww_bank_add(oww_ctx* h, const void* blob, size_t nbytes) {
    OWW_GUARD_BEGIN
    if (!h || !blob || nbytes < 32) return fail(OWW_EINVAL, "oww_bank_add: bad argument");
    if (!h->hx) return fail(OWW_ESTATE, "oww_bank_add: the head bank runs on the fp16-split heads kernels (use_mfma = 3) only");
    if (!h->committed || h->bank_K == 0) return fail(OWW_ESTATE, "oww_bank_add: needs oww_bank_configure before oww_commit, and a committed handle");
    const int32_t* hdr = (const int32_t*)blob;
    if (int rc = owb::add_header_check(hdr, h->TR)) return rc;
    const int T = hdr[1], H = hdr[2], has_ln = hdr[4];
    const size_t K = (size_t)T * 96;
    HeadHost hh{};                                   // (size and finiteness: the fixed heads' parser; the header is inside its ranges)
    if (int rc = parse_head_blob("oww_bank_add", blob, nbytes, h->TR, hh)) return rc;
    const float* q = hh.blob.data();
    int id = -1;
    for (int b = 0; b < h->bank_cap && id < 0; ++b) if (!h->bank[b].live) id = b;
    if (id < 0) return fail(OWW_EINVAL, "oww_bank_add: the bank is full (capacity %d)", h->bank_cap);
    HIPCHK(hipSetDevice(h->cfg.device));
    // ---- the packing of a fixed net of the same width (ht 4: <= 64 units, ht 8: <= 128), in an image of its own: w1hx | pack_hx_net
    NetHost net{};
    parse_dense_net(q, T, H, 1, has_ln, 1, net);
    const int ht = H <= 64 ? 4 : 8, HP = 16 * ht;
    HxNetPack pack;
    if (!hx_net_scales(net, ht, pack, h->probe_emb, h->probe_nb)) return fail(OWW_EINVAL, "oww_bank_add: head weights are not finite");
    HostBuf hb;
    std::vector<float> wcat(K * HP, 0.f), pk;
    std::vector<double> colmul(HP);
    place_w1(net, 0, HP, HP, pack.e1, wcat, colmul);
    pack_hx_w1(wcat.data(), (int)K, HP, colmul.data(), pk);
    const size_t o_w1 = hb.add(pk);
    const size_t w1_floats = pk.size();
    pack_hx_net(net, ht, true, hb, pack);
    DevBuf<float> d_img;                             // (the head's when the self-test passes, released on every other way out)
    HIPCHK(herr(d_img.alloc(hb.data.size())));
    if (copy_sync(d_img, hb.data.data(), hb.data.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
        return fail(OWW_EHIP, "oww_bank_add: weight upload failed");
    owh::BankHeadDev dv{};
    dv.w1hx = d_img + o_w1; dv.T = T; dv.ht = ht;
    dv.net = make_hx_net(net, ht, pack, d_img, nullptr, h->hx_efeat);
    // ---- self-test: the routed kernel on windows of the commit's probe embeddings against float64, the tolerance oww_commit holds
    //      fixed heads to (1e-3)
    std::vector<float> win;
    const int B = probe_windows(h->probe_emb, h->probe_nb, T, win);
    DevBuf<float> d_win, d_out; DevBuf<int> d_ent; DevBuf<owh::BankTile> d_til; DevBuf<owh::BankHeadDev> d_hd;
    std::vector<int> ent(B);
    for (int i = 0; i < B; ++i) ent[i] = i;
    std::vector<owh::BankTile> til;
    for (int o0 = 0; o0 < B; o0 += 128) til.push_back(owh::BankTile{0, o0, std::min(128, B - o0), 0});
    std::vector<float> got(B, 0.f);
    if (d_win.alloc(win.size()) || d_out.alloc(B) || d_ent.alloc(B) || d_til.alloc(til.size()) || d_hd.alloc(1))
        return fail(OWW_ENOMEM, "oww_bank_add: out of device memory (self-test)");
    if (copy_sync(d_win, win.data(), win.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
        copy_sync(d_ent, ent.data(), ent.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess ||
        copy_sync(d_til, til.data(), til.size() * sizeof(owh::BankTile), hipMemcpyHostToDevice) != hipSuccess ||
        copy_sync(d_hd, &dv, sizeof dv, hipMemcpyHostToDevice) != hipSuccess) return fail(OWW_EHIP, "oww_bank_add: self-test upload failed");
    const int flag_before = h->h_range ? *(volatile int*)h->h_range : 0;
    HIPCHK(hipStreamSynchronize(h->stream));
    owh::BankParams bp{};
    bp.feat = d_win; bp.ext = 1; bp.TR = T; bp.tiles = d_til; bp.entries = d_ent; bp.heads = d_hd; bp.K = 1;
    bp.raw = d_out; bp.range_flag = h->d_range; bp.fscale = std::ldexp(1.0f, h->hx_efeat);
    if (ht == 4) hipLaunchKernelGGL((owh::heads_bank_kernel<4, 4>), dim3((unsigned)til.size()), dim3(256), 0, h->stream, bp);
    else hipLaunchKernelGGL((owh::heads_bank_kernel<4, 8>), dim3((unsigned)til.size()), dim3(256), 0, h->stream, bp);
    int rc = 0;
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess ||
        copy_sync(got.data(), d_out, (size_t)B * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) rc = drained(h, fail(OWW_EHIP, "oww_bank_add: self-test run failed"));
    double err = 0.0;
    bool finite = true;
    for (int w = 0; w < B && !rc; ++w) {
        finite = finite && std::isfinite(got[w]);
        err = std::max(err, std::fabs((double)got[w] - bank_eval_f64(net, &win[(size_t)w * K])));
    }
    const bool raised = h->h_range && *(volatile int*)h->h_range && !flag_before;
    if (raised) *(volatile int*)h->h_range = 0;                 // (the self-test's own overflow is not the streams')
    if (!rc && (!finite || err > 1e-3 || raised))
        rc = fail(OWW_ERANGE, "oww_bank_add: with these weights the fp16-split heads kernel differs from a float64 evaluation by %.3g on the "
                  "commit's probe embeddings (tolerance 1e-3)%s: load the head as a fixed head of a use_mfma = 1 handle", err,
                  raised ? ", an activation left the f16 range" : "");
    if (rc) return rc;
    HIPCHK(copy_sync(h->d_bank_heads + id, &dv, sizeof dv, hipMemcpyHostToDevice));
    oww_ctx::BankHead& bh = h->bank[id];
    bh = oww_ctx::BankHead{};
    bh.live = true; bh.T = T; bh.hidden = H; bh.has_ln = has_ln; bh.ht = ht; bh.d_img = std::move(d_img); bh.dev = dv;
    bh.w1_bytes = w1_floats * sizeof(float);
    const int pat0 = 0; const float thr0 = NAN;
    HIPCHK(copy_sync(h->d_bank_pat + id, &pat0, sizeof pat0, hipMemcpyHostToDevice));
    HIPCHK(copy_sync(h->d_bank_thr + id, &thr0, sizeof thr0, hipMemcpyHostToDevice));
    return id;
    OWW_GUARD_END
}

int oww_bank_remove(oww_ctx* h, int32_t id) {
    OWW_GUARD_BEGIN
    if (!h || !h->committed || h->bank_K == 0) return fail(OWW_ESTATE, "oww_bank_remove: no bank on this handle");
    if (int rc = owb::head_id_check("oww_bank_remove", id, h->bank.data(), h->bank_cap)) return rc;
    HIPCHK(hipSetDevice(h->cfg.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    std::vector<int> changed;
    for (int i = 0; i < h->S * h->bank_K; ++i) if (h->bank_sub[i] == id) { h->bank_sub[i] = -1; changed.push_back(i); }
    if (!changed.empty()) HIPCHK(copy_sync(h->d_bank_sub, h->bank_sub.data(), h->bank_sub.size() * sizeof(int), hipMemcpyHostToDevice));
    if (int rc = bank_clear(h, changed)) return rc;
    if (int rc = sv_drop_bank(h, changed)) return rc;
    h->bank[id] = oww_ctx::BankHead{};               // (releases the head's image)
    return bank_route(h);
    OWW_GUARD_END
}

int oww_bank_set_postproc(oww_ctx* h, int32_t id, int32_t patience, float threshold) {
    OWW_GUARD_BEGIN
    if (!h || !h->committed || h->bank_K == 0) return fail(OWW_ESTATE, "oww_bank_set_postproc: no bank on this handle");
    if (int rc = owb::head_id_check("oww_bank_set_postproc", id, h->bank.data(), h->bank_cap)) return rc;
    HIPCHK(hipSetDevice(h->cfg.device));
    HIPCHK(copy_async(h->d_bank_pat + id, &patience, sizeof patience, hipMemcpyHostToDevice, h->stream));
    HIPCHK(copy_async(h->d_bank_thr + id, &threshold, sizeof threshold, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->bank[id].patience = patience; h->bank[id].threshold = threshold;
    return OWW_OK;
    OWW_GUARD_END
}

int oww_subscribe(oww_ctx* h, const int32_t* stream_ids, int32_t n, const int32_t* bank_ids) {
    OWW_GUARD_BEGIN
    if (!h || !h->committed || h->bank_K == 0) return fail(OWW_ESTATE, "oww_subscribe: no bank on this handle");
    if (n < 0 || (n > 0 && (!stream_ids || !bank_ids))) return fail(OWW_EINVAL, "oww_subscribe: bad argument");
    const int K = h->bank_K;
    if (int rc = owb::subscribe_check(stream_ids, n, bank_ids, h->S, K, h->bank.data(), h->bank_cap)) return rc;
    HIPCHK(hipSetDevice(h->cfg.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    std::vector<int> changed;
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < K; ++k) {
            const size_t at = (size_t)stream_ids[i] * K + k;
            const int b = bank_ids[(size_t)i * K + k];
            if (h->bank_sub[at] != b) { h->bank_sub[at] = b; changed.push_back((int)at); }    // a new head in the slot starts afresh
        }
    if (changed.empty()) return OWW_OK;
    HIPCHK(copy_sync(h->d_bank_sub, h->bank_sub.data(), h->bank_sub.size() * sizeof(int), hipMemcpyHostToDevice));
    if (int rc = bank_clear(h, changed)) return rc;
    if (int rc = sv_drop_bank(h, changed)) return rc;
    return bank_route(h);
    OWW_GUARD_END
}

int oww_bank_scores(oww_ctx* h, float* out) {
    OWW_GUARD_BEGIN
    if (!h || !h->committed || h->bank_K == 0) return fail(OWW_ESTATE, "oww_bank_scores: no bank on this handle");
    if (!out) return fail(OWW_EINVAL, "oww_bank_scores: null output");
    HIPCHK(hipSetDevice(h->cfg.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(copy_sync(out, h->d_bank_scores, (size_t)h->S * h->bank_K * sizeof(float), hipMemcpyDeviceToHost));
    return range_check(h, "oww_bank_scores");
    OWW_GUARD_END
}

const float* oww_bank_scores_dev(const oww_ctx* h) { return h && h->committed ? h->d_bank_scores : nullptr; }

int oww_bank_routing(oww_ctx* h, int32_t info[6], double* weight_bytes) {
    OWW_GUARD_BEGIN
    if (!h || !h->committed || h->bank_K == 0) return fail(OWW_ESTATE, "oww_bank_routing: no bank on this handle");
    if (info)
        for (int c = 0; c < 2; ++c) { info[3 * c] = h->bank_rt.ntiles[c]; info[3 * c + 1] = h->bank_rt.wg[c]; info[3 * c + 2] = h->bank_rt.entries_n[c]; }
    if (weight_bytes) *weight_bytes = h->bank_rt.wbytes;
    return OWW_OK;
    OWW_GUARD_END
}

// ---- per-stream custom verifiers ------------------------------------------------------------------------------------------------------
int oww_verifier_configure(oww_ctx* h, int32_t capacity) {
    OWW_GUARD_BEGIN
    if (!h) return fail(OWW_EINVAL, "null handle");
    if (h->committed) return fail(OWW_ESTATE, "oww_verifier_configure: call before oww_commit");
    if (capacity < 1 || capacity > 65536) return fail(OWW_EINVAL, "oww_verifier_configure: capacity = %d (1..65536)", capacity);
    h->vpool_cap = capacity;
    return OWW_OK;
    OWW_GUARD_END
}

int oww_verifier_add(oww_ctx* h, const float* w, int32_t n_w, float bias) {
    OWW_GUARD_BEGIN
    if (!h || !h->committed || h->vpool_cap == 0) return fail(OWW_ESTATE, "oww_verifier_add: needs oww_verifier_configure before oww_commit, and a committed handle");
    if (!w || n_w <= 0 || n_w % OWW_EMB_DIM) return fail(OWW_EINVAL, "oww_verifier_add: %d weights (a verifier has T x 96)", n_w);
    const int T = n_w / OWW_EMB_DIM;
    if (T > h->TR) return fail(OWW_EINVAL, "oww_verifier_add: T = %d exceeds the handle's feature ring (%d rows)", T, h->TR);
    for (int i = 0; i < n_w; ++i) if (!std::isfinite(w[i])) return fail(OWW_EINVAL, "oww_verifier_add: weight %d is not finite", i);
    if (!std::isfinite(bias)) return fail(OWW_EINVAL, "oww_verifier_add: the bias is not finite");
    int id = -1;
    for (int v = 0; v < h->vpool_cap && id < 0; ++v) if (h->vpool_T[v] == 0) id = v;
    if (id < 0) return fail(OWW_EINVAL, "oww_verifier_add: the verifier pool is full (capacity %d)", h->vpool_cap);
    HIPCHK(hipSetDevice(h->cfg.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(copy_sync(h->d_vpool_w + (size_t)id * h->vpool_stride, w, (size_t)n_w * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(copy_sync(h->d_vpool_b + id, &bias, sizeof bias, hipMemcpyHostToDevice));
    h->vpool_T[id] = T;
    return id;
    OWW_GUARD_END
}

int oww_verifier_remove(oww_ctx* h, int32_t id) {
    OWW_GUARD_BEGIN
    if (!h || !h->committed || h->vpool_cap == 0) return fail(OWW_ESTATE, "oww_verifier_remove: no verifier pool on this handle");
    if (id < 0 || id >= h->vpool_cap || h->vpool_T[id] == 0) return fail(OWW_EINVAL, "oww_verifier_remove: %d is not a pool verifier", id);
    HIPCHK(hipSetDevice(h->cfg.device));
    HIPCHK(hipStreamSynchronize(h->stream));     // in-flight steps may still read the entry and the list
    for (auto* tab : {&h->vasg_fix, &h->vasg_bank})
        for (int& v : *tab) if (v == id) { v = OWW_VERIFIER_DEFAULT; --h->vasg_n; }
    h->vpool_T[id] = 0;
    return sv_rebuild(h);
    OWW_GUARD_END
}

// ---- fitting custom verifiers on the device (owwhip_fit.h; host side: owwhip_fit_host.h) ---------------------------------------------
int oww_verifier_fit(oww_ctx* h, const float* windows, int windows_on_device, const int64_t* offsets, const uint8_t* labels, int32_t U, int32_t T, float C,
                     oww_fit_result* out) {
    OWW_GUARD_BEGIN
    if (!h) return fail(OWW_EINVAL, "null handle");
    if (int rc = owf::check_args(h->committed, h->vpool_cap, windows, offsets, labels, U, T, h->TR, C, out)) return rc;
    if (U == 0) return OWW_OK;
    std::vector<oww_fit_result> res((size_t)U);
    owf::classify(offsets, labels, U, res.data());
    if (int rc = owf::assign_ids(h->vpool_T, U, res.data())) return rc;
    std::vector<int> run, Ns;                          // the problems that go to the device, and their N
    for (int u = 0; u < U; ++u) if (res[u].status == OWW_FIT_OK) { run.push_back(u); Ns.push_back((int)(offsets[u + 1] - offsets[u])); }
    const long long D = (long long)T * OWW_EMB_DIM;
    long long budget = owf::kDefaultBudget;
    if (const char* e = getenv("OWW_FIT_SCRATCH_BYTES")) budget = std::max(1ll, atoll(e));
    const std::vector<owf::Slab> slabs = owf::slab_plan(Ns, D, budget, windows_on_device != 0);
    HIPCHK(hipSetDevice(h->cfg.device));
    auto& F = h->fit;
    std::vector<owf::Record> recs;
    for (const owf::Slab& sl : slabs) {
        const int np = sl.last - sl.first;
        std::vector<owf::Problem> prob((size_t)np);
        std::vector<unsigned char> y((size_t)sl.rows);
        long long row = 0, koff = 0;
        for (int i = 0; i < np; ++i) {
            const int u = run[sl.first + i], N = Ns[sl.first + i];
            prob[i] = owf::Problem{windows_on_device ? (long long)offsets[u] * D : row * D, row, koff, row, N, res[u].id, u, 0};
            memcpy(y.data() + row, labels + offsets[u], (size_t)N);
            row += N; koff += (long long)N * N;
        }
        const std::vector<owf::Tile> tiles = owf::tile_map(Ns, sl.first, sl.last);
        const size_t zn = (size_t)sl.rows * D;
        bool ok = grow(h, F.zh, zn) == hipSuccess && grow(h, F.zl, zn) == hipSuccess && grow(h, F.K, (size_t)sl.k_floats) == hipSuccess &&
                  grow(h, F.a, (size_t)sl.rows) == hipSuccess && grow(h, F.b, (size_t)np) == hipSuccess && grow(h, F.mu, (size_t)np * D) == hipSuccess &&
                  grow(h, F.sd, (size_t)np * D) == hipSuccess && grow(h, F.y, (size_t)sl.rows) == hipSuccess && grow(h, F.flag, (size_t)np) == hipSuccess &&
                  grow(h, F.rec, (size_t)np) == hipSuccess && grow(h, F.prob, (size_t)np) == hipSuccess && grow(h, F.tiles, tiles.size()) == hipSuccess;
        if (ok && !windows_on_device) ok = grow(h, F.x, zn) == hipSuccess;
        if (!ok) return fail(OWW_ENOMEM, "oww_verifier_fit: out of device memory for a slab of %d problems (%lld windows)", np, sl.rows);
        if (!windows_on_device)                         // the slab's windows, problem after problem (skipped problems leave gaps in the call's)
            for (int i = 0; i < np; ++i)
                HIPCHK(copy_async(F.x + prob[i].x_off, windows + (size_t)offsets[prob[i].u] * D, (size_t)prob[i].N * D * sizeof(float), hipMemcpyHostToDevice, h->stream));
        HIPCHK(copy_async(F.prob, prob.data(), prob.size() * sizeof(owf::Problem), hipMemcpyHostToDevice, h->stream));
        HIPCHK(copy_async(F.tiles, tiles.data(), tiles.size() * sizeof(owf::Tile), hipMemcpyHostToDevice, h->stream));
        HIPCHK(copy_async(F.y, y.data(), y.size(), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemsetAsync(F.flag, 0, (size_t)np * sizeof(int), h->stream));
        owfk::FitParams p{};
        p.prob = F.prob; p.x = windows_on_device ? windows : F.x.get(); p.y = F.y;
        p.zh = reinterpret_cast<_Float16*>(F.zh.get()); p.zl = reinterpret_cast<_Float16*>(F.zl.get());
        p.mu = F.mu; p.sd = F.sd; p.K = F.K; p.a = F.a; p.b = F.b; p.flag = F.flag; p.rec = F.rec; p.tiles = F.tiles;
        p.n_tiles = (int)tiles.size(); p.n_prob = np; p.D = (int)D; p.C = C;
        p.pool_w = h->d_vpool_w; p.pool_b = h->d_vpool_b; p.pool_stride = h->vpool_stride;
        hipLaunchKernelGGL(owfk::fit_stats_kernel, dim3((unsigned)((D + 255) / 256), np), dim3(256), 0, h->stream, p);
        hipLaunchKernelGGL(owfk::fit_gram_kernel, dim3((unsigned)((tiles.size() + 3) / 4)), dim3(256), 0, h->stream, p);
        hipLaunchKernelGGL(owfk::fit_solve_kernel, dim3(np), dim3(owfk::kSolveThreads), 0, h->stream, p);
        hipLaunchKernelGGL(owfk::fit_fold_kernel, dim3(np), dim3(256), 0, h->stream, p);
        HIPCHK(hipGetLastError());
        recs.resize((size_t)np);
        HIPCHK(copy_async(recs.data(), F.rec, (size_t)np * sizeof(owf::Record), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));       // the slab's scratch and host staging are free again; its records are here
        for (int i = 0; i < np; ++i) {
            oww_fit_result& r = res[prob[i].u];
            r.status = recs[i].status; r.iterations = recs[i].iterations; r.residual = recs[i].residual;
            if (r.status == OWW_FIT_OK) h->vpool_T[r.id] = T;     // live, exactly as after oww_verifier_add
            else r.id = -1;
        }
    }
    for (int u = 0; u < U; ++u) out[u] = res[u];
    return OWW_OK;
    OWW_GUARD_END
}

int oww_verifier_get(oww_ctx* h, int32_t id, float* w, int32_t n_w, float* bias) {
    OWW_GUARD_BEGIN
    if (!h || !h->committed || h->vpool_cap == 0) return fail(OWW_ESTATE, "oww_verifier_get: no verifier pool on this handle");
    if (id < 0 || id >= h->vpool_cap || h->vpool_T[id] == 0) return fail(OWW_EINVAL, "oww_verifier_get: %d is not a pool verifier", id);
    if (!w || !bias || n_w != h->vpool_T[id] * OWW_EMB_DIM)
        return fail(OWW_EINVAL, "oww_verifier_get: room for %d weights, verifier %d has %d x 96", n_w, id, h->vpool_T[id]);
    HIPCHK(hipSetDevice(h->cfg.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(copy_sync(w, h->d_vpool_w + (size_t)id * h->vpool_stride, (size_t)n_w * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(copy_sync(bias, h->d_vpool_b + id, sizeof(float), hipMemcpyDeviceToHost));
    return OWW_OK;
    OWW_GUARD_END
}

// ---- training bank heads on the device (owwhip_train.h; host side: owwhip_train_host.h) ---------------------------------------------
int64_t oww_train_param_count(int32_t T, int32_t hidden) {
    if (T < 1 || hidden < 16 || hidden > 128 || hidden % 16) return 0;
    return owt::layout(T, hidden).n;
}

extern "C++" {
template <int NT>
static int train_launch_step(oww_ctx* h, const owtk::TrainParams& p, const owt::Plan& pl, int U) {
    const size_t lds = (size_t)owtk::fwd_lds_floats(NT) * sizeof(float);
    hipLaunchKernelGGL(owtk::train_fwd_kernel<NT>, dim3(pl.n_tiles, U), dim3(256), lds, h->stream, p);
    hipLaunchKernelGGL(owtk::train_w1_kernel<NT>, dim3(pl.w1_groups, U), dim3(256), 0, h->stream, p);
    hipLaunchKernelGGL(owtk::train_small_kernel, dim3(U), dim3(256), 0, h->stream, p);
    return 0;
}
template <int NT>
static hipError_t train_set_lds() {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(owtk::train_fwd_kernel<NT>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               owtk::fwd_lds_floats(NT) * (int)sizeof(float));
}
}  // extern "C++"
#define OWW_TRAIN_NT(nt, CALL)                                                                                                        \
    switch (nt) {                                                                                                                     \
        case 1: CALL(1); break; case 2: CALL(2); break; case 3: CALL(3); break; case 4: CALL(4); break;                               \
        case 5: CALL(5); break; case 6: CALL(6); break; case 7: CALL(7); break; default: CALL(8); break;                              \
    }

int oww_train_begin(oww_ctx* h, int32_t U, int32_t T, int32_t hidden, const float* params) {
    OWW_GUARD_BEGIN
    if (!h) return fail(OWW_EINVAL, "null handle");
    if (int rc = owt::check_begin(h->committed, h->train.open, U, T, hidden, h->TR, params)) return rc;
    HIPCHK(hipSetDevice(h->cfg.device));
    auto& S = h->train;
    const owt::Layout L = owt::layout(T, hidden);
    const size_t n = (size_t)U * L.stride;
    if (grow(h, S.par, n) != hipSuccess || grow(h, S.am, n) != hipSuccess || grow(h, S.av, n) != hipSuccess || grow(h, S.cnt, (size_t)U) != hipSuccess)
        return fail(OWW_ENOMEM, "oww_train_begin: out of device memory for %d problems of %lld parameters", U, L.n);
#define OWW_TRAIN_LDS(NT) HIPCHK(train_set_lds<NT>())
    OWW_TRAIN_NT(hidden / 16, OWW_TRAIN_LDS)
#undef OWW_TRAIN_LDS
    std::vector<float> stage(n, 0.f);
    for (int u = 0; u < U; ++u) memcpy(stage.data() + (size_t)u * L.stride, params + (size_t)u * L.n, (size_t)L.n * sizeof(float));
    const std::vector<owt::Counters> cnt((size_t)U, owt::Counters{1, 0, 0, 0});
    HIPCHK(copy_async(S.par, stage.data(), n * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIPCHK(copy_async(S.cnt, cnt.data(), cnt.size() * sizeof(owt::Counters), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemsetAsync(S.am, 0, n * sizeof(float), h->stream));
    HIPCHK(hipMemsetAsync(S.av, 0, n * sizeof(float), h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    S.U = U; S.T = T; S.D = hidden; S.L = L; S.P = 0; S.open = true;
    return OWW_OK;
    OWW_GUARD_END
}

int oww_train_set_pool(oww_ctx* h, const float* pool, int pool_on_device, int64_t P) {
    OWW_GUARD_BEGIN
    if (!h) return fail(OWW_EINVAL, "null handle");
    auto& S = h->train;
    if (int rc = owt::check_pool(S.open, pool, P, S.T)) return rc;
    HIPCHK(hipSetDevice(h->cfg.device));
    const size_t n = (size_t)P * S.L.F;
    if (grow(h, S.pool, n) != hipSuccess) { S.P = 0; return fail(OWW_ENOMEM, "oww_train_set_pool: out of device memory for %lld windows", (long long)P); }
    HIPCHK(copy_async(S.pool, pool, n * sizeof(float), pool_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    S.P = P;
    return OWW_OK;
    OWW_GUARD_END
}

int oww_train_steps(oww_ctx* h, int32_t K, int32_t n_batch, const int32_t* idx, const uint8_t* y, int shared_tables, int tables_on_device,
                    const double* lr, const float* neg_weight, oww_train_record* out) {
    OWW_GUARD_BEGIN
    if (!h) return fail(OWW_EINVAL, "null handle");
    auto& S = h->train;
    if (!S.open) return fail(OWW_ESTATE, "oww_train_steps: no training session on this handle");
    if (K < 1 || K > owt::kMaxSteps || n_batch < 1 || n_batch > owt::kMaxBatch || !idx || !y)      // (the sizes below rest on these)
        return owt::check_steps(true, S.P, S.U, K, n_batch, idx, y, shared_tables, lr, neg_weight, out);
    HIPCHK(hipSetDevice(h->cfg.device));
    const size_t total = (size_t)(shared_tables ? 1 : S.U) * K * n_batch;
    std::vector<int32_t> idx_h;
    std::vector<uint8_t> y_h;
    if (tables_on_device) {                      // checked on the host like host tables: a copy back, behind whatever wrote them on this stream
        idx_h.resize(total); y_h.resize(total);
        HIPCHK(hipStreamSynchronize(h->stream));
        HIPCHK(copy_sync(idx_h.data(), idx, total * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIPCHK(copy_sync(y_h.data(), y, total, hipMemcpyDeviceToHost));
    }
    const int32_t* idx_c = tables_on_device ? idx_h.data() : idx;
    const uint8_t* y_c = tables_on_device ? y_h.data() : y;
    if (int rc = owt::check_steps(true, S.P, S.U, K, n_batch, idx_c, y_c, shared_tables, lr, neg_weight, out)) return rc;
    const owt::Plan pl = owt::plan(S.U, S.T, S.D, n_batch);
    const size_t nrec = (size_t)S.U * K;
    if (grow(h, S.idx, total) != hipSuccess || grow(h, S.y, total) != hipSuccess || grow(h, S.lr, (size_t)K) != hipSuccess || grow(h, S.nw, (size_t)K) != hipSuccess ||
        grow(h, S.dz1, (size_t)pl.dz1) != hipSuccess || grow(h, S.part, (size_t)pl.part) != hipSuccess || grow(h, S.tcount, (size_t)pl.tile_words) != hipSuccess ||
        grow(h, S.tloss, (size_t)pl.tile_words) != hipSuccess || grow(h, S.rec, nrec) != hipSuccess)
        return fail(OWW_ENOMEM, "oww_train_steps: out of device memory for %d problems x %d rows", S.U, pl.n_pad);
    HIPCHK(copy_async(S.idx, idx_c, total * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(copy_async(S.y, y_c, total, hipMemcpyHostToDevice, h->stream));
    HIPCHK(copy_async(S.lr, lr, (size_t)K * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(copy_async(S.nw, neg_weight, (size_t)K * sizeof(float), hipMemcpyHostToDevice, h->stream));
    owtk::TrainParams p{};
    p.par = S.par; p.am = S.am; p.av = S.av; p.cnt = S.cnt; p.pool = S.pool; p.idx = S.idx; p.y = S.y; p.lr = S.lr; p.nw = S.nw;
    p.dz1 = S.dz1; p.part = S.part; p.tcount = S.tcount; p.tloss = S.tloss; p.rec = S.rec;
    p.tab_stride = shared_tables ? 0 : (long long)K * n_batch;
    p.stride = S.L.stride; p.small = S.L.small;
    p.P = (int)S.P; p.F = (int)S.L.F; p.D = S.D; p.K = K; p.n_batch = n_batch; p.n_tiles = pl.n_tiles; p.n_pad = pl.n_pad;
    for (int k = 0; k < K; ++k) {                // the K steps back to back on the handle's stream: no host round trip between them
        p.k = k;
#define OWW_TRAIN_STEP(NT) train_launch_step<NT>(h, p, pl, S.U)
        OWW_TRAIN_NT(S.D / 16, OWW_TRAIN_STEP)
#undef OWW_TRAIN_STEP
    }
    HIPCHK(hipGetLastError());
    std::vector<owt::StepRecord> recs(nrec);
    HIPCHK(copy_async(recs.data(), S.rec, nrec * sizeof(owt::StepRecord), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (size_t i = 0; i < nrec; ++i) { out[i].loss = recs[i].loss; out[i].m = recs[i].m; }
    return OWW_OK;
    OWW_GUARD_END
}

int oww_train_get(oww_ctx* h, int32_t u, float* params, int64_t n_params) {
    OWW_GUARD_BEGIN
    if (!h) return fail(OWW_EINVAL, "null handle");
    auto& S = h->train;
    if (!S.open) return fail(OWW_ESTATE, "oww_train_get: no training session on this handle");
    if (u < 0 || u >= S.U) return fail(OWW_EINVAL, "oww_train_get: problem %d of %d", u, S.U);
    if (!params || n_params != S.L.n) return fail(OWW_EINVAL, "oww_train_get: room for %lld floats, a record has %lld", (long long)n_params, S.L.n);
    HIPCHK(hipSetDevice(h->cfg.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(copy_sync(params, S.par + (size_t)u * S.L.stride, (size_t)S.L.n * sizeof(float), hipMemcpyDeviceToHost));
    return OWW_OK;
    OWW_GUARD_END
}

int oww_train_end(oww_ctx* h) {
    OWW_GUARD_BEGIN
    if (!h) return fail(OWW_EINVAL, "null handle");
    auto& S = h->train;
    if (!S.open) return fail(OWW_ESTATE, "oww_train_end: no training session on this handle");
    HIPCHK(hipSetDevice(h->cfg.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    S = oww_ctx::TrainSession{};
    return OWW_OK;
    OWW_GUARD_END
}

// ---- validating, checkpointing and merging the heads of a session (owwhip_autotrain.h; host side: owwhip_autotrain_host.h) ------------
extern "C++" {
template <int NT>
static int train_launch_eval(oww_ctx* h, const owak::EvalParams& p, int n_tiles, int U) {
    const size_t lds = (size_t)owak::eval_lds_floats(NT) * sizeof(float);
    hipLaunchKernelGGL(owak::train_eval_kernel<NT>, dim3(U, n_tiles), dim3(256), lds, h->stream, p);
    return 0;
}
}  // extern "C++"

int oww_train_new_sequence(oww_ctx* h) {
    OWW_GUARD_BEGIN
    if (!h) return fail(OWW_EINVAL, "null handle");
    auto& S = h->train;
    if (int rc = owa::check_new_sequence(S.open)) return rc;
    HIPCHK(hipSetDevice(h->cfg.device));
    // the counters of every problem, behind the steps that wrote them: the optimizer's step count is read back and kept
    std::vector<owt::Counters> cnt((size_t)S.U);
    HIPCHK(copy_async(cnt.data(), S.cnt, cnt.size() * sizeof(owt::Counters), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (auto& c : cnt) { c.acc_steps = 1; c.acc_samples = 0; }
    HIPCHK(copy_async(S.cnt, cnt.data(), cnt.size() * sizeof(owt::Counters), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return OWW_OK;
    OWW_GUARD_END
}

int oww_train_set_eval_pool(oww_ctx* h, const float* pool, int pool_on_device, int64_t P) {
    OWW_GUARD_BEGIN
    if (!h) return fail(OWW_EINVAL, "null handle");
    auto& S = h->train;
    if (int rc = owa::check_eval_pool(S.open, pool, P, S.T)) return rc;
    HIPCHK(hipSetDevice(h->cfg.device));
    const size_t n = (size_t)P * S.L.F;
    HIPCHK(hipStreamSynchronize(h->stream));
    if (n > S.epool.capacity()) {                // a larger pool: the old one stays until the new one exists, so a refusal leaves it
        DevBuf<float> fresh;
        if (fresh.alloc(n) != 0) {
            (void)hipGetLastError();
            return fail(OWW_ENOMEM, "oww_train_set_eval_pool: out of device memory for %lld windows", (long long)P);
        }
        S.epool = std::move(fresh);
        S.EP = 0;                                // (the old windows are gone from here on; the copy below fills the new ones)
    }
    HIPCHK(copy_async(S.epool, pool, n * sizeof(float), pool_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    S.EP = P;
    return OWW_OK;
    OWW_GUARD_END
}

int oww_train_eval(oww_ctx* h, int32_t source, int32_t n, const int32_t* idx, const uint8_t* y, int shared_tables, int tables_on_device,
                   float* scores, oww_train_counts* counts) {
    OWW_GUARD_BEGIN
    if (!h) return fail(OWW_EINVAL, "null handle");
    auto& S = h->train;
    if (int rc = owa::check_eval_head(S.open, S.EP, S.C, source, n, idx, y, counts)) return rc;      // (the sizes below rest on these)
    HIPCHK(hipSetDevice(h->cfg.device));
    const owa::EvalPlan pl = owa::eval_plan(S.U, n, shared_tables, scores != nullptr);
    const size_t total = (size_t)pl.table;
    std::vector<int32_t> idx_h;
    std::vector<uint8_t> y_h;
    if (tables_on_device) {                      // checked on the host like host tables, as oww_train_steps does
        idx_h.resize(total); y_h.resize(total);
        HIPCHK(hipStreamSynchronize(h->stream));
        HIPCHK(copy_sync(idx_h.data(), idx, total * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIPCHK(copy_sync(y_h.data(), y, total, hipMemcpyDeviceToHost));
    }
    const int32_t* idx_c = tables_on_device ? idx_h.data() : idx;
    const uint8_t* y_c = tables_on_device ? y_h.data() : y;
    if (int rc = owa::check_eval(true, S.EP, S.C, S.U, source, n, idx_c, y_c, shared_tables, counts)) return rc;
    const size_t ncnt = (size_t)S.U * owa::kCounts;
    if (grow(h, S.eidx, total) != hipSuccess || grow(h, S.ey, total) != hipSuccess || grow(h, S.ecounts, ncnt) != hipSuccess ||
        (scores && grow(h, S.escores, (size_t)pl.scores) != hipSuccess))
        return fail(OWW_ENOMEM, "oww_train_eval: out of device memory for %d problems x %d slots", S.U, n);
    HIPCHK(copy_async(S.eidx, idx_c, total * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(copy_async(S.ey, y_c, total, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemsetAsync(S.ecounts, 0, ncnt * sizeof(int), h->stream));
    owak::EvalParams p{};
    p.par = source < 0 ? (const float*)S.par : (const float*)S.ckpt + (size_t)source * S.U * S.L.stride;
    p.pool = S.epool; p.idx = S.eidx; p.y = S.ey; p.scores = scores ? (float*)S.escores : nullptr; p.counts = S.ecounts;
    p.tab_stride = shared_tables ? 0 : (long long)n;
    p.stride = S.L.stride; p.P = (int)S.EP; p.F = (int)S.L.F; p.n = n;
#define OWW_TRAIN_EVAL(NT) train_launch_eval<NT>(h, p, pl.n_tiles, S.U)
    OWW_TRAIN_NT(S.D / 16, OWW_TRAIN_EVAL)
#undef OWW_TRAIN_EVAL
    HIPCHK(hipGetLastError());
    std::vector<int32_t> cnt_h(ncnt);
    HIPCHK(copy_async(cnt_h.data(), S.ecounts, ncnt * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (scores) HIPCHK(copy_async(scores, S.escores, (size_t)pl.scores * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int u = 0; u < S.U; ++u) {
        const int32_t* c = cnt_h.data() + (size_t)u * owa::kCounts;
        counts[u] = oww_train_counts{c[0], c[1], c[2], c[3], c[4]};
    }
    return OWW_OK;
    OWW_GUARD_END
}

int oww_train_checkpoints(oww_ctx* h, int32_t C) {
    OWW_GUARD_BEGIN
    if (!h) return fail(OWW_EINVAL, "null handle");
    auto& S = h->train;
    long long floats = 0;
    if (int rc = owa::check_checkpoints(S.open, C, S.U, S.L.stride, &floats)) return rc;
    HIPCHK(hipSetDevice(h->cfg.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    DevBuf<float> slots;                         // the old slots stay until the new ones exist
    if (slots.alloc((size_t)floats) != 0) {
        (void)hipGetLastError();
        return fail(OWW_ENOMEM, "oww_train_checkpoints: out of device memory for %d slots x %d problems of %lld parameters", C, S.U, S.L.n);
    }
    HIPCHK(hipMemsetAsync(slots, 0, (size_t)floats * sizeof(float), h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    S.ckpt = std::move(slots);
    S.C = C;
    return OWW_OK;
    OWW_GUARD_END
}

int oww_train_snapshot(oww_ctx* h, const int32_t* slot) {
    OWW_GUARD_BEGIN
    if (!h) return fail(OWW_EINVAL, "null handle");
    auto& S = h->train;
    if (int rc = owa::check_snapshot(S.open, S.C, S.U, slot)) return rc;
    HIPCHK(hipSetDevice(h->cfg.device));
    if (grow(h, S.slot, (size_t)S.U) != hipSuccess) return fail(OWW_ENOMEM, "oww_train_snapshot: out of device memory for %d slot numbers", S.U);
    HIPCHK(copy_async(S.slot, slot, (size_t)S.U * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    const unsigned groups = (unsigned)((S.L.stride / 4 + 255) / 256);
    hipLaunchKernelGGL(owak::train_snapshot_kernel, dim3(groups, S.U), dim3(256), 0, h->stream, (const float*)S.par, (float*)S.ckpt, (const int*)S.slot,
                       S.L.stride, S.U);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));     // `slot` is the caller's memory
    return OWW_OK;
    OWW_GUARD_END
}

int oww_train_average(oww_ctx* h, const uint8_t* sel, int32_t dst) {
    OWW_GUARD_BEGIN
    if (!h) return fail(OWW_EINVAL, "null handle");
    auto& S = h->train;
    if (int rc = owa::check_average(S.open, S.C, sel, dst)) return rc;
    HIPCHK(hipSetDevice(h->cfg.device));
    const size_t n = (size_t)S.U * S.C;
    if (grow(h, S.sel, n) != hipSuccess) return fail(OWW_ENOMEM, "oww_train_average: out of device memory for %d x %d selections", S.U, S.C);
    HIPCHK(copy_async(S.sel, sel, n, hipMemcpyHostToDevice, h->stream));
    const unsigned groups = (unsigned)((S.L.stride / 4 + 255) / 256);
    hipLaunchKernelGGL(owak::train_average_kernel, dim3(groups, S.U), dim3(256), 0, h->stream, (const float*)S.par, (float*)S.ckpt,
                       (const unsigned char*)S.sel, S.L.stride, S.U, S.C, dst);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    return OWW_OK;
    OWW_GUARD_END
}

int oww_train_get_slot(oww_ctx* h, int32_t u, int32_t slot, float* params, int64_t n_params) {
    OWW_GUARD_BEGIN
    if (!h) return fail(OWW_EINVAL, "null handle");
    auto& S = h->train;
    if (int rc = owa::check_get_slot(S.open, S.C, S.U, u, slot, params, n_params, S.L.n)) return rc;
    HIPCHK(hipSetDevice(h->cfg.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(copy_sync(params, S.ckpt + ((size_t)slot * S.U + u) * S.L.stride, (size_t)S.L.n * sizeof(float), hipMemcpyDeviceToHost));
    return OWW_OK;
    OWW_GUARD_END
}

// shared body of oww_assign_verifiers (bank = false: `col` is a score column) and oww_bank_assign_verifiers (bank = true: a slot)
static int assign_impl(oww_ctx* h, bool bank, int32_t col, const int32_t* stream_ids, int32_t n, const int32_t* verifier_ids,
                       const float* thresholds) {
    const char* fn = bank ? "oww_bank_assign_verifiers" : "oww_assign_verifiers";
    if (!h || !h->committed || h->vpool_cap == 0) return fail(OWW_ESTATE, "%s: no verifier pool on this handle (oww_verifier_configure)", fn);
    if (bank && h->bank_K == 0) return fail(OWW_ESTATE, "%s: no bank on this handle", fn);
    const int ncol = bank ? h->bank_K : h->NL;
    int colT = 0;                                      // feature rows of the column's model
    if (!bank) for (const auto& hh : h->heads) if (col >= hh.out_col && col < hh.out_col + hh.n_out) colT = hh.T;
    auto model_T = [&](int s) {                        // ... or of the head in the stream's slot (< 0: the slot is empty)
        if (!bank) return colT;
        const int b = h->bank_sub[(size_t)s * h->bank_K + col];
        return b < 0 ? -1 : h->bank[b].T;
    };
    if (int rc = owsv::assign_check(fn, bank, col, ncol, stream_ids, n, verifier_ids, thresholds, h->S, h->vpool_T, model_T)) return rc;
    HIPCHK(hipSetDevice(h->cfg.device));
    HIPCHK(hipStreamSynchronize(h->stream));           // ordered behind every queued step (oww_submit)
    owsv::assign_apply(bank ? h->vasg_bank : h->vasg_fix, bank ? h->vthr_bank : h->vthr_fix, h->vasg_n, col, ncol, stream_ids, n, verifier_ids, thresholds);
    return sv_rebuild(h);
}

int oww_assign_verifiers(oww_ctx* h, int32_t label, const int32_t* stream_ids, int32_t n, const int32_t* verifier_ids, const float* thresholds) {
    OWW_GUARD_BEGIN
    return assign_impl(h, false, label, stream_ids, n, verifier_ids, thresholds);
    OWW_GUARD_END
}

int oww_bank_assign_verifiers(oww_ctx* h, int32_t slot, const int32_t* stream_ids, int32_t n, const int32_t* verifier_ids, const float* thresholds) {
    OWW_GUARD_BEGIN
    return assign_impl(h, true, slot, stream_ids, n, verifier_ids, thresholds);
    OWW_GUARD_END
}

int oww_verifier_stats(oww_ctx* h, int64_t out[2]) {
    OWW_GUARD_BEGIN
    if (!h || !h->committed) return fail(OWW_ESTATE, "oww_verifier_stats: handle not committed");
    if (!out) return fail(OWW_EINVAL, "oww_verifier_stats: null output");
    unsigned long long n_eval = 0;
    if (h->d_sv_eval) {
        HIPCHK(hipSetDevice(h->cfg.device));
        HIPCHK(hipStreamSynchronize(h->stream));
        HIPCHK(copy_sync(&n_eval, h->d_sv_eval, sizeof n_eval, hipMemcpyDeviceToHost));
    }
    out[0] = h->vasg_n;
    out[1] = (int64_t)n_eval;
    return OWW_OK;
    OWW_GUARD_END
}

// ---- stream state records -------------------------------------------------------------------------------------------------------------
#define OWW_STATE_ENTER(fn)                                                                                     \
    if (!h) return fail(OWW_EINVAL, fn ": null handle");                                                        \
    if (!h->committed) return fail(OWW_ESTATE, fn ": handle not committed");                                    \
    HIPCHK(hipSetDevice(h->cfg.device));                                                                        \
    if (int rc__ = state_layout(h)) return rc__;

int oww_state_info(oww_ctx* h, size_t* record_bytes, uint64_t* fingerprint) {
    OWW_GUARD_BEGIN
    OWW_STATE_ENTER("oww_state_info")
    if (record_bytes) *record_bytes = (size_t)h->st_record_words * 4;
    if (fingerprint) *fingerprint = h->st_fp;
    return OWW_OK;
    OWW_GUARD_END
}

int oww_state_export(oww_ctx* h, const int32_t* stream_ids, int32_t n, void* out, int out_on_device) {
    OWW_GUARD_BEGIN
    OWW_STATE_ENTER("oww_state_export")
    if (n < 0 || (n > 0 && (!stream_ids || !out))) return fail(OWW_EINVAL, "oww_state_export: bad argument");
    if (n == 0) return OWW_OK;
    if (int rc = ows::state_check_ids(h->S, "oww_state_export", "the", stream_ids, n, false)) return rc;
    if (out_on_device && (reinterpret_cast<uintptr_t>(out) & 15)) return fail(OWW_EINVAL, "oww_state_export: a device buffer must be 16-byte aligned");
    std::vector<int> buf;
    ows::StateList L;
    ows::state_list_build(h->st_levels, stream_ids, n, buf, L);
    if (!out_on_device) if (int rc = state_stage(h, n)) return rc;
    if (int rc = state_lists_upload(h, buf)) return rc;
    uint32_t* rec = out_on_device ? static_cast<uint32_t*>(out) : h->d_st_stage;
    if (int rc = state_xfer<false>(h, L, rec)) return rc;
    if (!out_on_device) HIPCHK(copy_async(out, rec, (size_t)n * h->st_record_words * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));           // the host list was the upload's source; a host buffer is complete on return
    return OWW_OK;
    OWW_GUARD_END
}

int oww_state_import(oww_ctx* h, const int32_t* stream_ids, int32_t n, const void* in, int in_on_device) {
    OWW_GUARD_BEGIN
    OWW_STATE_ENTER("oww_state_import")
    if (n < 0 || (n > 0 && (!stream_ids || !in))) return fail(OWW_EINVAL, "oww_state_import: bad argument");
    if (n == 0) return OWW_OK;
    if (int rc = ows::state_check_ids(h->S, "oww_state_import", "the", stream_ids, n, true)) return rc;
    if (in_on_device && (reinterpret_cast<uintptr_t>(in) & 15)) return fail(OWW_EINVAL, "oww_state_import: a device buffer must be 16-byte aligned");
    // every header is checked before anything changes
    const size_t rb = (size_t)h->st_record_words * 4;
    std::vector<uint32_t> hdr((size_t)n * ows::kHeaderWords);
    if (in_on_device) {
        HIPCHK(hipMemcpy2DAsync(hdr.data(), ows::kHeaderWords * 4, in, rb, ows::kHeaderWords * 4, n, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    } else {
        for (int i = 0; i < n; ++i) memcpy(&hdr[(size_t)i * ows::kHeaderWords], static_cast<const char*>(in) + (size_t)i * rb, ows::kHeaderWords * 4);
    }
    if (int rc = ows::state_check_headers(h->st_record_words, h->st_fp, hdr.data(), n)) return rc;
    std::vector<int> buf;
    ows::StateList L;
    ows::state_list_build(h->st_levels, stream_ids, n, buf, L);
    if (!in_on_device) if (int rc = state_stage(h, n)) return rc;
    if (int rc = state_lists_upload(h, buf)) return rc;
    uint32_t* rec = in_on_device ? static_cast<uint32_t*>(const_cast<void*>(in)) : h->d_st_stage;
    if (!in_on_device) HIPCHK(copy_async(rec, in, (size_t)n * rb, hipMemcpyHostToDevice, h->stream));
    if (int rc = state_xfer<true>(h, L, rec)) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));           // the host list and a host buffer were copy sources
    return OWW_OK;
    OWW_GUARD_END
}

int oww_move_streams(oww_ctx* h, const int32_t* src, const int32_t* dst, int32_t n) {
    OWW_GUARD_BEGIN
    OWW_STATE_ENTER("oww_move_streams")
    if (n < 0 || (n > 0 && (!src || !dst))) return fail(OWW_EINVAL, "oww_move_streams: bad argument");
    if (n == 0) return OWW_OK;
    if (int rc = ows::state_check_ids(h->S, "oww_move_streams", "source", src, n, false)) return rc;
    if (int rc = ows::state_check_ids(h->S, "oww_move_streams", "destination", dst, n, true)) return rc;
    std::vector<int> buf;
    ows::StateList Ls, Ld;
    ows::state_list_build(h->st_levels, src, n, buf, Ls);
    ows::state_list_build(h->st_levels, dst, n, buf, Ld);
    if (int rc = state_stage(h, n)) return rc;
    if (int rc = state_lists_upload(h, buf)) return rc;
    // every read happens before any write: gather all sources into the staging records, then scatter them
    if (int rc = state_xfer<false>(h, Ls, h->d_st_stage)) return rc;
    if (int rc = state_xfer<true>(h, Ld, h->d_st_stage)) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));           // also: no queued step still reads the routing table or the verifier list
    // what the library keeps per stream on the host travels too: subscriptions and verifier assignments leave the source slot (a
    // source that is nobody's destination is left empty / at the default) and arrive at the destination; one rebuild per table
    if (h->bank_K == 0 && h->vpool_cap == 0) return OWW_OK;
    std::vector<int32_t> dsorted(dst, dst + n);
    std::sort(dsorted.begin(), dsorted.end());
    auto travel = [&](auto& tab, int width, auto empty) -> bool {
        if (width == 0 || tab.empty()) return false;
        const auto old = tab;
        for (int i = 0; i < n; ++i)
            if (!std::binary_search(dsorted.begin(), dsorted.end(), src[i]))
                for (int k = 0; k < width; ++k) tab[(size_t)src[i] * width + k] = empty;
        for (int i = 0; i < n; ++i)
            for (int k = 0; k < width; ++k) tab[(size_t)dst[i] * width + k] = old[(size_t)src[i] * width + k];
        return tab != old;
    };
    if (h->bank_K > 0 && travel(h->bank_sub, h->bank_K, -1)) {
        HIPCHK(copy_sync(h->d_bank_sub, h->bank_sub.data(), h->bank_sub.size() * sizeof(int), hipMemcpyHostToDevice));
        if (int rc = bank_route(h)) return rc;           // (a moved slot does not restart: its ring and counter came with the record)
    }
    if (h->vpool_cap > 0) {
        bool ch = travel(h->vasg_fix, h->NL, (int)OWW_VERIFIER_DEFAULT);
        ch = travel(h->vthr_fix, h->NL, 0.f) || ch;
        ch = travel(h->vasg_bank, h->bank_K, (int)OWW_VERIFIER_DEFAULT) || ch;
        ch = travel(h->vthr_bank, h->bank_K, 0.f) || ch;
        if (ch) {
            h->vasg_n = owsv::count_assigned(h->vasg_fix, h->vasg_bank);
            if (int rc = sv_rebuild(h)) return rc;
        }
    }
    return OWW_OK;
    OWW_GUARD_END
}

int oww_comm_id(void* id) {
    OWW_GUARD_BEGIN
    if (!id) return fail(OWW_EINVAL, "oww_comm_id: null argument");
    if (int rc = rccl_load()) return rc;
    RCCLCHK(g_rccl.GetUniqueId(id));
    return OWW_OK;
    OWW_GUARD_END
}

int oww_comm_init(oww_ctx* h, const void* id, int32_t rank, int32_t world) {
    OWW_GUARD_BEGIN
    if (!h || !h->committed) return fail(OWW_ESTATE, "oww_comm_init: handle not committed");
    if (!id || world < 1 || rank < 0 || rank >= world) return fail(OWW_EINVAL, "oww_comm_init: bad argument (rank %d of %d)", rank, world);
    if (h->comm) return fail(OWW_ESTATE, "oww_comm_init: the handle already has a communicator");
    if (int rc = rccl_load()) return rc;
    HIPCHK(hipSetDevice(h->cfg.device));
    RcclId uid;
    memcpy(uid.b, id, sizeof uid.b);
    void* comm = nullptr;
    RCCLCHK(g_rccl.CommInitRank(&comm, world, uid, rank));
    h->comm = comm; h->comm_rank = rank; h->comm_world = world;
    return OWW_OK;
    OWW_GUARD_END
}

int oww_gather_scores(oww_ctx* h, float* out, const int32_t* counts) {
    OWW_GUARD_BEGIN
    if (!h || !h->committed) return fail(OWW_ESTATE, "oww_gather_scores: handle not committed");
    if (!h->comm) return fail(OWW_ESTATE, "oww_gather_scores: call oww_comm_init first");
    if (!counts) return fail(OWW_EINVAL, "oww_gather_scores: counts is null");
    if (counts[h->comm_rank] != h->S) return fail(OWW_EINVAL, "oww_gather_scores: counts[%d] = %d, this handle owns %d streams", h->comm_rank, counts[h->comm_rank], h->S);
    if (h->comm_rank == 0 && !out) return fail(OWW_EINVAL, "oww_gather_scores: rank 0 needs the output buffer");
    HIPCHK(hipSetDevice(h->cfg.device));
    const size_t NL = (size_t)h->NL;
    if (NL == 0) return OWW_OK;
    // one grouped exchange on the handle's stream (ordered after the step that produced d_scores): every rank sends its [S_r][NL]
    // block to rank 0 -- rank 0 to itself as well, so the path is the same RCCL kernel at any world size
    RCCLCHK(g_rccl.GroupStart());
    int rc_send = g_rccl.Send(h->d_scores, (size_t)h->S * NL, 7 /* ncclFloat32 */, 0, h->comm, h->stream);
    int rc_recv = 0;
    if (h->comm_rank == 0) {
        size_t off = 0;
        for (int r = 0; r < h->comm_world && !rc_recv; ++r) {
            if (counts[r] < 0) { rc_recv = -1; break; }
            if (counts[r] > 0) rc_recv = g_rccl.Recv(out + off, (size_t)counts[r] * NL, 7, r, h->comm, h->stream);
            off += (size_t)counts[r] * NL;
        }
    }
    const int rc_end = g_rccl.GroupEnd();
    if (rc_send) RCCLCHK(rc_send);
    if (rc_recv < 0) return fail(OWW_EINVAL, "oww_gather_scores: negative count");
    if (rc_recv) RCCLCHK(rc_recv);
    RCCLCHK(rc_end);
    return OWW_OK;
    OWW_GUARD_END
}

int oww_comm_count(oww_ctx* h, int32_t* ranks) {
    OWW_GUARD_BEGIN
    if (!h || !ranks) return fail(OWW_EINVAL, "oww_comm_count: null argument");
    if (!h->comm) return fail(OWW_ESTATE, "oww_comm_count: call oww_comm_init first");
    int n = 0;
    RCCLCHK(g_rccl.CommCount(h->comm, &n));
    *ranks = n;
    return OWW_OK;
    OWW_GUARD_END
}

int oww_comm_destroy(oww_ctx* h) {
    OWW_GUARD_BEGIN
    if (!h) return OWW_OK;
    if (h->comm) { (void)hipSetDevice(h->cfg.device); (void)hipStreamSynchronize(h->stream); }
    comm_release(h);
    return OWW_OK;
    OWW_GUARD_END
}

}  // extern "C"
