/*
 * owwhip.h -- C ABI of libowwhip.so: the MI355X (gfx950) streaming wake-word path.
 *
 * This is the drop-in boundary for the ONE hot path of dscripka/openWakeWord:
 *   int16 PCM 16 kHz -> log-mel -> speech-embedding CNN -> wake-word heads -> post-processing.
 * The reference crosses this boundary through three onnxruntime / LiteRT closures
 *   melspec_model_predict        openwakeword/utils.py:87  (122-136 for tflite)
 *   embedding_model_predict      openwakeword/utils.py:93  (147-161)
 *   model_prediction_function[]  openwakeword/model.py:137-138, 158-159 (116-119, 174-175)
 * and keeps all per-stream state in Python objects (utils.py:163-170, model.py:198).  Here the state
 * of S concurrent streams lives in HBM and one call advances every stream by one 80 ms step.
 *
 * Conventions: plain C, opaque handle, every function returns 0 on success and a negative OWW_E*
 * code on failure (message via oww_last_error()); nothing throws across the ABI.  One handle = one
 * GPU; calls on one handle must be serialised by the caller (the reference object is single-threaded
 * too).  "dev" pointers are HIP device pointers valid on the handle's device; "host" pointers are
 * ordinary host memory.  All float data is IEEE fp32, row-major, C order.
 */
#ifndef OWWHIP_H
#define OWWHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OWW_ABI_VERSION 6

#define OWW_OK            0
#define OWW_EINVAL       -1   /* bad argument */
#define OWW_EHIP         -2   /* HIP runtime error */
#define OWW_ESTATE       -3   /* call out of order (e.g. step before weights committed) */
#define OWW_ENOMEM       -4
#define OWW_ERANGE       -5   /* fp16-split kernels (use_mfma = 3): an activation left the f16 range; sticky, see oww_range_status */

#define OWW_CHUNK        1280 /* samples per 80 ms step          (utils.py:417-434) */
#define OWW_MEL_BINS       32 /* melspectrogram.onnx output bins (utils.py:271)     */
#define OWW_MEL_PER_CHUNK   8 /* new mel rows per step                 */
#define OWW_WINDOW         76 /* mel rows per embedding window   (utils.py:225,440) */
#define OWW_EMB_DIM        96 /* embedding_model.onnx output     (utils.py:323)     */
#define OWW_SCORE_RING     30 /* prediction_buffer maxlen        (model.py:198)     */
#define OWW_MAX_HEADS      16
#define OWW_MAX_HEAD_BLOCKS 8    /* hidden blocks of one head network (train.py:73); the released models have 1 */
#define OWW_MAX_LABELS     32
#define OWW_MAX_CALL_CHUNKS 4096 /* longest oww_step call: 4096 x 80 ms = 5.5 minutes of audio per stream */

typedef struct oww_ctx oww_ctx;

typedef struct oww_config {
    int32_t device;        /* HIP device ordinal */
    int32_t n_streams;     /* S: concurrent audio streams owned by this handle */
    int32_t max_chunks;    /* largest n_chunks a single oww_step may carry (>=1) */
    int32_t feature_ring;  /* rows of the per-stream feature ring; 0 = max head T (>=16) */
    int32_t use_mfma;      /* kernel family of the embedding CNN and the heads:
                              3 = register-resident kernels, fp32 products as three f16 MFMAs (hi/lo split, fp32 accumulate;
                                  default path, agrees with the fp32 families to fp32 round-off),
                              1 = register-resident kernels on the exact fp32 MFMA,
                              2 = LDS-tiled fp32-MFMA kernels, 0 = plain-VALU kernels of the LDS-tiled dataflow */
    int32_t debug_layers;  /* 1 = keep per-layer CNN outputs of the last step for oww_debug_read */
    void*   stream;        /* hipStream_t to launch on; NULL = a stream owned by the handle */
} oww_config;

/* ---- lifetime -------------------------------------------------------------------------------- */
int  oww_abi_version(void);
/* "src=<16 hex digits> arch=gfx950": the hash of the sources this binary was built from (openwakeword_amd/_build.py: source_hash).
 * Profiles committed under profiles/ carry the same hash, so a measurement can be tied to the kernels it was taken on. */
const char* oww_build_info(void);
const char* oww_last_error(void);
int  oww_create(const oww_config* cfg, oww_ctx** out);
int  oww_destroy(oww_ctx* h);

/* ---- weights (replace the .onnx/.tflite files of openwakeword/__init__.py:8-51) ----------------
 * Host blobs, copied.  Layouts:
 *  mel   : float hann[400]; int32 start[32]; float taps[32][16]          (window + sparse mel filterbank)
 *  embed : for each of the 20 conv layers in graph order: float w[kh][kw][cin][cout] (Keras HWIO),
 *          then for layers 0..18: float scale[cout]; float shift[cout]   (inference BatchNorm folded)
 *  head  : int32 hdr[8] = {kind(0 binary,1 gated,2 multiclass), T, hidden, n_out, has_layernorm, extra_blocks,0,0}
 *          then per net (1 net; 2 for gated): w1[T*96][hidden] b1[hidden] (ln1_g ln1_b [hidden] if
 *          has_layernorm), then 1 + extra_blocks times { w2[hidden][hidden] b2 (ln2_g ln2_b) }, then w3[hidden][n_out] b3[n_out].
 *          extra_blocks = 0 is the network of every released model (train.py:27,67: n_blocks = 1); train.py's Net takes any
 *          n_blocks (train.py:73): extra_blocks = n_blocks - 1, from -1 (no hidden block) to OWW_MAX_HEAD_BLOCKS - 1.  Nets with
 *          other than one block are evaluated by the generic heads kernel (any kernel family), not by the MFMA head kernels.
 *          In the default family (use_mfma = 3) one-block nets of up to 64 hidden units and one sigmoid output run on the f16-split
 *          heads kernel, and ungated one-block nets of up to 128 hidden units / 8 outputs (the multiclass `timer` model,
 *          docs/models/timers.md:9-27) on its wide form; everything else on the generic kernel.
 *  head, recurrent (train.py:85-98, model_type "rnn"): hdr = {3, T (<= 64), 64, n_out, 0, 0, 0, 0}; then for LSTM layer 0 (input 96) and 1
 *          (input 128), for direction forward and reverse: w[in + 64][256] (rows x ; h, columns i | f | g | o -- torch's gate order),
 *          b[256] (= b_ih + b_hh); then w_out[128][n_out], b_out[n_out].  Output = Sigmoid (n_out = 1) or ReLU + softmax of the
 *          linear layer on the last time step (out[:, -1]).
 */
int  oww_load_mel(oww_ctx* h, const void* blob, size_t nbytes);
int  oww_load_embedding(oww_ctx* h, const void* blob, size_t nbytes);
int  oww_add_head(oww_ctx* h, const void* blob, size_t nbytes);     /* returns head index >= 0 */
/* oww_commit: pack + upload, allocate state, derive reset state, then reset all.  For the default kernel family (use_mfma = 3) it also
 * (1) calibrates: a scratch handle of the exact-fp32 family runs the all-ones mel history and 32 probe streams x 16 frames (silence,
 *     noise RMS 30..32767, full-scale square waves) on the same weights; from every layer's largest |activation| each layer gets a
 *     power-of-two scale under which its f16-split operands keep full precision, and BatchNorm is folded into the packed weights;
 * (2) self-tests: the probes are replayed on the f16-split kernels and embeddings / raw head outputs compared with the fp32 run.
 * Weights the split cannot carry within the north-star tolerance (1e-3) -- the reference's fp32 graphs have no such limit,
 * utils.py:84-93 -- are REFUSED here with OWW_ERANGE (message names the deviation; use use_mfma = 1 for them) instead of scoring
 * differently later.  Adds ~0.05-0.3 s to the call.  (OWW_NO_COMMIT_SELFTEST=1 in the environment skips step (2): development only.) */
int  oww_commit(oww_ctx* h);
/* Optional, before oww_commit, use_mfma = 3 only (ignored by the fp32 families): calibration audio of the caller's domain -- int16
 * [n_streams][n_frames * 1280], host pointer, copied.  oww_commit derives the fp16-split kernels' scale ladder from, and runs its
 * f16x3-vs-fp32 self-test on, the built-in synthetic probes (silence, noise at five levels, square waves) PLUS this audio, cut into
 * 16-frame segments (at most 224 of them are used).  The reference's fp32 graphs have no range to calibrate (utils.py:84-93); the
 * Python layer passes speech (the reference's three fixture clips at several gains) by default.  pcm = NULL clears the set. */
int  oww_set_calibration(oww_ctx* h, const int16_t* pcm, int32_t n_streams, int32_t n_frames);
/* What oww_commit measured and decided (use_mfma = 3; any pointer may be NULL): absmax[l] = largest |activation| of CNN layer l over
 * the probe set on the exact-fp32 kernels; exps[l] = the layer's power-of-two scale exponent, exps[20] = the exponent the heads' GEMM
 * applies to the features; n_probe_streams = 32 built-in + the caller's 16-frame segments; selftest = {max |embedding - fp32|,
 * max |embedding|, max |raw score - fp32|} of the fp16-split replay of the probes. */
int  oww_calibration_info(oww_ctx* h, float absmax[20], int32_t exps[21], int32_t* n_probe_streams, float selftest[3]);
int  oww_n_labels(const oww_ctx* h);  /* total score columns = sum of n_out over heads */

/* ---- per-stream state (AudioFeatures.reset utils.py:172-178 + Model.reset model.py:226-230) -----
 * stream_ids == NULL resets every stream.  init_features (host, [feature_ring][96], oldest row first)
 * seeds the feature ring the way the reference seeds it with embeddings of random audio
 * (utils.py:169); NULL = zeros. */
int  oww_reset(oww_ctx* h, const int32_t* stream_ids, int32_t n, const float* init_features);

/* ---- post-processing options of Model.predict (model.py:340-359); arrays of oww_n_labels() -------
 * patience[i] <= 0 and debounce_frames <= 0 disable the respective rule for label i. */
int  oww_set_postproc(oww_ctx* h, const int32_t* patience, const float* threshold, int32_t debounce_frames);

/* ---- custom verifier models (model.py:320-328; trained by custom_verifier_model.py:95-113) on the device ----------------------
 * The reference re-scores a label whose base score reaches `threshold` (custom_verifier_threshold, default 0.1) with a pickled
 * scikit-learn pipeline: flatten -> StandardScaler -> LogisticRegression over the last T feature rows of the label's model
 * (T x 96 values, oldest row first).  Scaler and regression fold into one affine map, which is what this entry takes:
 * w[T*96] = coef / scale, bias = intercept - sum(coef * mean / scale); the label then reads sigmoid(w . features + bias)
 * (= predict_proba(...)[0][-1]) whenever its head output is >= threshold, before the post-processing rules.  w == NULL removes
 * the label's verifier.  Weights and bias must be finite (OWW_EINVAL, as oww_verifier_add).  Host pointers; call after oww_commit. */
int  oww_set_verifier(oww_ctx* h, int32_t label, const float* w, int32_t n_w, float bias, float threshold);

/* ---- VAD gate of Model.predict (model.py:366-381) for the batched path -------------------------------------------------
 * Two ways to feed the gate.  (1) External network (the reference's silero_vad.onnx is a release asset whose graph is not in the
 * reference checkout, so it cannot be built into this library): the caller supplies one VAD score per stream and step -- the mean
 * over the step's 640-sample sub-frames that VAD.__call__ appends (vad.py:98-130) -- with oww_push_vad.  (2) A network on the device:
 * oww_load_vad below (a structural stand-in with the same interface and state).  Either way the library keeps the per-stream
 * score ring and applies the gate: when the largest
 * of the scores pushed 5..7 steps ago (ring[-7:-4]; nothing during the first four steps) is below `threshold`, every label of
 * that stream reads 0 for the step (the 30-deep score ring keeps the ungated value, as in the reference).  threshold <= 0
 * switches the gate off (default).  Call oww_push_vad BEFORE the oww_step / oww_submit of the same frame; vad_scores is
 * fp32 [S], host or device.  Like Model.reset(), oww_reset leaves the VAD ring alone. */
int  oww_set_vad_threshold(oww_ctx* h, float threshold);
int  oww_push_vad(oww_ctx* h, const float* vad_scores, int on_device);
/* Voice-activity NETWORK on the device (BASELINE configs[4]: "VAD gate fused into the per-frame HIP pipeline").  Silero's graph
 * is unavailable (see above), so this loads a structural STAND-IN with the interface and state the reference fixes around the
 * network (vad.py:98-130: 640-sample sub-frames / 32767, recurrent state h, c [2, 1, 64] carried from call to call, one score
 * per sub-frame, the mean per predict() call appended to the ring): |STFT| (256-sample Hann frames, hop 64, bins 1..128) ->
 * log(1 + gain |X|) -> 4 x [Conv1d(k=3, pad 1) + ReLU] 128->16 (stride 1), 16->32 (2), 32->32 (2), 32->64 (1) -> 2-layer LSTM(64)
 * -> ReLU -> Linear(64->1) -> sigmoid, mean over time.  Blob (call before oww_commit): int32 hdr[8] = {1, 256, 64, 128, 64, 0, 0, 0};
 * float gain; float hann[256]; per conv: w[3][cin][cout], b[cout]; per LSTM layer: w[128][256] (rows x ; h, columns i | f | g | o),
 * b[256] (= b_ih + b_hh); float wd[64]; float bd.  Once loaded, every oww_step / oww_submit (n_chunks must be 1) runs the network
 * on the frame's two sub-frames of every stream and pushes the mean score into the stream's ring; oww_push_vad is then refused.
 * oww_get_vad copies the scores of the last step (host fp32 [S]) -- it waits for the handle's stream, so with submitted steps in flight
 * "the last step" is the NEWEST submitted one, not the one the last oww_collect delivered: read it with nothing in flight when it has to
 * belong to the collected scores; oww_reset_vad zeroes recurrent state and score history of the
 * listed streams (NULL = all) -- oww_reset does not, exactly like Model.reset() leaves Model.vad alone (model.py:226-230). */
int  oww_load_vad(oww_ctx* h, const void* blob, size_t nbytes);
int  oww_get_vad(oww_ctx* h, float* out);
int  oww_reset_vad(oww_ctx* h, const int32_t* stream_ids, int32_t n);

/* ---- the hot loop: one Model.predict per stream (model.py:232-386) --------------------------------
 * pcm: int16 [S][n_chunks*1280], stream-major.  scores: fp32 [S][n_labels] or NULL.
 * *_on_device: 0 = host pointer (copied on the handle's stream), 1 = device pointer.
 * n_chunks > 1 reproduces the reference's multi-chunk call: one mel pass over the whole span
 * (single top_db clamp), one embedding + head evaluation per chunk, max over chunks (model.py:287-298).
 * n_chunks may exceed oww_config.max_chunks (up to OWW_MAX_CALL_CHUNKS): the call is then evaluated in slices of max_chunks chunks
 * behind one extra pass of the mel kernel that finds the CALL's maximum, so that the clamp floor is still the reference's single
 * "max - 80 dB" over the whole call (utils.py:387-401: one run of melspectrogram.onnx per call); such a call is synchronous when pcm
 * is a host pointer, and is refused with the on-device VAD network (one chunk per step).
 * Asynchronous on the handle's stream unless scores is a host pointer.
 * A DEVICE pcm pointer should be 16-byte aligned: the fused front end loads eight samples at a time; any other alignment (a slice of
 * a larger int16 buffer) is accepted and takes the separate mel launch with scalar sample loads -- same scores to fp32 round-off
 * (1e-6), about 10 % slower. */
int  oww_step(oww_ctx* h, const int16_t* pcm, int pcm_on_device, int32_t n_chunks,
              float* scores, int scores_on_device);
int  oww_sync(oww_ctx* h);
/* The same one-chunk step for the streams a serving edge actually has a full 80 ms chunk for (clients of
 * examples/web/streaming_server.py:49-66 arrive, stall and leave independently; in the reference each of them simply does not
 * call predict() while it has no audio).  stream_on: uint8 [S], 1 = the stream takes part: exactly oww_step for it; 0 = the
 * stream sits the step out: none of its state moves (sample tail, conv histories, feature and score rings, frame counters,
 * VAD state) and its row of `scores` repeats its previous step's values; its 1280 PCM samples are not read.  A stream
 * stepped k times through any interleaving of masked steps is in the state k plain steps leave it in, bit for bit.
 * Cost: with a HOST mask of which at most 7/8 of the streams take part (8 n <= 7 S), only the stage groups (1 / 2 / 4 / 8 streams of a wave) that
 * hold a participating stream are launched and the heads run on the participants alone, so the step costs roughly in proportion to
 * the participation (streams sharing a group with a participant are computed and not stored); a device-resident mask, or more than
 * 7/8 of the streams, runs the full launches, whose stores skip the streams that sit out; a host mask with nobody on launches nothing.  Both register-resident kernel families take masked steps (use_mfma = 3 and the exact
 * fp32 family 1, so weights the fp16 split refuses at commit can still be served; heads of any form); the proportional cost is the
 * default family's (fused front end, heads of the [T,96] -> 64 -> 64 -> 1 form) -- every other combination runs full launches whose
 * stores skip the streams that sit out.  The LDS-tiled families (use_mfma = 2, 0) return OWW_EINVAL. */
int  oww_step_masked(oww_ctx* h, const int16_t* pcm, int pcm_on_device, const uint8_t* stream_on, int stream_on_on_device,
                     float* scores, int scores_on_device);
/* Range guard of the default kernel family (use_mfma = 3 evaluates every fp32 product as three f16 MFMAs on hi/lo-split
 * operands, so an activation with |x| >= 65520 cannot be represented).  The reference's fp32 graphs have no such limit
 * (onnxruntime CPU kernels, utils.py:84-93), so instead of scoring silently differently the kernels test one accumulator
 * per position tile and layer for the NaN such an operand produces and raise a sticky per-handle flag.  Once raised,
 * oww_step / oww_submit / oww_collect / oww_sync / oww_embed* return OWW_ERANGE (a step issued with device-resident
 * scores is asynchronous: the error surfaces on the next call that looks).  oww_range_status waits for the handle's
 * stream and returns OWW_OK or OWW_ERANGE; clear != 0 lowers the flag (after e.g. resetting the offending streams).
 * The exact-fp32 family (use_mfma = 1) never raises it. */
int  oww_range_status(oww_ctx* h, int clear);
/* Which streams: after OWW_ERANGE, first_stream / n_streams name the contiguous streams of (one of) the wave(s) that saw the
 * out-of-range value -- the offender is among them -- so that a server can oww_reset just those and clear the flag instead of
 * restarting every stream; (-1, 0) when the flag is down or the position is not known (a step over a participant list). */
int  oww_range_where(oww_ctx* h, int32_t* first_stream, int32_t* n_streams);

/* ---- host-fed pipeline: the same step with PCM arriving in host memory every 80 ms (the serving edge of
 *      examples/web/streaming_server.py:32-70 and detect_from_microphone.py: audio is produced on the host) ----------
 * oww_submit enqueues  H2D(pcm) -> step -> D2H(scores)  and returns at once: the upload runs on its own stream, so the
 * PCM of step t+1 crosses PCIe while the kernels of step t execute; oww_collect blocks until the OLDEST submitted step
 * has delivered and copies its fp32 [S][n_labels] scores to `scores` (host).  At most two steps may be in flight
 * (submit, submit, collect, submit, collect, ...); a third submit returns OWW_ESTATE.  `pcm` must stay valid and
 * unmodified until the matching oww_collect returns; use page-locked memory (oww_host_alloc, hipHostMalloc,
 * torch pin_memory) -- pageable memory works but makes the upload synchronous.  Results are identical to oww_step. */
int  oww_submit(oww_ctx* h, const int16_t* pcm, int32_t n_chunks);
/* oww_submit for the streams with stream_on[s] != 0 only (one chunk; see oww_step_masked): the serving edge's pipelined form.
 * stream_on: host uint8 [S], read before the call returns. */
int  oww_submit_masked(oww_ctx* h, const int16_t* pcm, const uint8_t* stream_on);
int  oww_collect(oww_ctx* h, float* scores);
int  oww_host_alloc(void** out, size_t nbytes);   /* page-locked host memory for PCM / score buffers */
int  oww_host_free(void* p);
const float* oww_scores_dev(const oww_ctx* h);     /* device [S][n_labels], valid until the next step */
/* raw head outputs of the last step, BEFORE post-processing (what model_prediction_function returned,
 * model.py:313-317; max over chunks for n_chunks > 1): host fp32 [S][n_labels].  Blocking.  Lets a host
 * shim run the reference's own post-processing (Model.predict with short / unaligned calls). */
int  oww_get_raw(oww_ctx* h, float* out);
/* Rate conversion of every stream's message on the device, the batched form of the serving example's per-message
 * resampy.resample(data, sample_rate, 16000) (examples/web/streaming_server.py:57-58): a polyphase FIR,
 *   out[s][j] = sat_int16(rint(sum_k taps[(j p) % q][k] * in[s][(j p) / q + k - n_taps / 2 + 1])),   samples outside the message = 0,
 * with p / q = input rate / 16000 in lowest terms, taps float [q][n_taps] on the host (n_taps even; the Kaiser-windowed sinc bank of
 * openwakeword_amd/resample.py::design, or any other) and n_out = n_in * q / p.  in: int16 [S][n_in], out: int16 [S][n_out], host or
 * device.  Stateless per call, like the example; asynchronous when out is a device pointer. */
int  oww_resample(oww_ctx* h, const int16_t* in, int in_on_device, int32_t n_in, int32_t p, int32_t q, const float* taps, int32_t n_taps,
                  int16_t* out, int out_on_device, int32_t n_out);

/* ---- stateful stream ingest: G.711 / PCM16 decode and CONTINUOUS rate conversion on the device, straight into the step ------------
 * oww_resample above converts every message on its own, like the serving example: each message is zero-padded on both sides, so
 * every 80 ms frame starts and ends inside the filter's transient (35.9 dB SNR against conversion of the whole recording at 8 kHz
 * with 640-sample messages).  These entries keep the filter running across messages, per stream, and take what telephony gateways
 * deliver (G.711 at 8 kHz) without a host decode.
 * Definition.  X = every decoded sample a stream has received since its last reset, message after message; p / q = input rate /
 * 16000 in lowest terms; taps float [q][n_taps] (n_taps even; resample.py::design or any other).  Output sample J of the stream is
 *   out[J] = sat_int16(rint(sum_k taps[(J p) % q][k] * X[(J p) / q + k - (n_taps - 1)])),   X[i] = 0 for i < 0,
 * k over the row padded with zeros to a multiple of 4, in order, an fp32 fmaf chain started at 0: oww_resample's definition applied to
 * the whole recording behind n_taps / 2 zeros, bit for bit.  So the latency is n_taps / 2 INPUT samples (13 samples = 1.6 ms at 8 kHz
 * with resample.py's bank), no output depends on a sample that has not arrived, and how the recording is cut into messages changes
 * nothing.  A message must hold a whole number of output samples, (n_in * q) % p == 0 (OWW_EINVAL otherwise; every standard rate has
 * such an 80 ms frame: 640 at 8 kHz, 882 at 11.025, 1764 at 22.05, 3528 at 44.1, 3840 at 48 kHz); every message then starts at filter
 * phase 0, n_out = n_in * q / p, and the only per-stream state is the last n_taps - 1 decoded samples.
 * Encodings: OWW_ENC_PCM16 (int16), OWW_ENC_ULAW / OWW_ENC_ALAW (one byte per sample, the G.711 expansion to 16 bit):
 *   mu-law  u = ~b; t = (((u & 15) << 3) + 0x84) << ((u >> 4) & 7); value = u & 0x80 ? 0x84 - t : t - 0x84
 *   A-law   a = b ^ 0x55; t = (a & 15) << 4; seg = (a >> 4) & 7; seg 0: t += 8; seg 1: t += 0x108; else t = (t + 0x108) << (seg - 1);
 *           value = a & 0x80 ? t : -t
 * p = q = 1 with n_taps = 0 (taps ignored) means decode only: no filter, no history.
 *   oww_ingest_configure  after oww_commit.  Allocates the history int16 [S][Hpad] (Hpad = n_taps - 1 rounded up to 8 samples, zeroed),
 *                       a 16-byte aligned staging buffer for the 16 kHz output (grown on demand) and uploads the padded bank.  Calling
 *                       it again reconfigures and zeroes every history.  Unknown encoding, odd n_taps, n_taps > 4096, q > 65536: OWW_EINVAL.
 *   oww_ingest          in: [S][n_in] in the configured encoding, host or device.  out: int16 [S][n_out], host or device; NULL = the
 *                       handle's staging buffer, which oww_ingest_dev returns (valid until the next ingest call).  stream_on: uint8 [S]
 *                       or NULL (host or device); a stream with stream_on[s] == 0 is not read, its history does not move and its output
 *                       row is not written.  One workgroup converts one stream's message out of LDS: a message whose history + samples
 *                       exceed 96 KB as floats (about 24,000 samples) is refused with OWW_EINVAL naming the numbers.  Asynchronous when
 *                       every pointer is a device pointer (or NULL); a host `out` with a mask is copied run by run of participants.
 *   oww_step_ingest     oww_ingest into the staging buffer, then oww_step (n_out / 1280 chunks; stream_on == NULL) or oww_step_masked
 *                       (one chunk) from that device pointer: the 16 kHz audio never leaves the device, and the staging buffer is
 *                       aligned, so the step takes its fast path.  n_out must be a positive multiple of 1280 (OWW_EINVAL naming it;
 *                       nothing has moved then).  With oww_use_graph the ingest launch precedes the replay on the handle's stream.
 * oww_reset also zeroes the ingest history of the streams it resets (a new caller starts from silence); oww_move_streams,
 * oww_state_export and oww_state_import carry it: once ingest is configured the record has one more flat section of Hpad / 2 words
 * behind the existing ones, and the fingerprint also covers encoding, p, q and the bank's bytes (configuring ingest rebuilds the
 * layout table).  A handle that never configures ingest has the records, fingerprint, allocations and launches it had before.
 * Cost model: bandwidth.  Per stream and 80 ms step at 8 kHz mu-law 640 B in, 2,560 B out and 2 x 64 B of history against about
 * 36 k FMAs out of LDS; loads are 16 codes (or 8 samples) per lane, stores 8 outputs per lane, the history moves in 16-byte pieces
 * (rows that do not start on 16-byte boundaries take element-wise accesses).  Not counted by oww_kernel_times. */
#define OWW_ENC_PCM16 0
#define OWW_ENC_ULAW  1
#define OWW_ENC_ALAW  2
int  oww_ingest_configure(oww_ctx* h, int32_t encoding, int32_t p, int32_t q, const float* taps, int32_t n_taps);
int  oww_ingest(oww_ctx* h, const void* in, int in_on_device, int32_t n_in, const uint8_t* stream_on, int stream_on_on_device,
                int16_t* out, int out_on_device);
const int16_t* oww_ingest_dev(const oww_ctx* h);
int  oww_step_ingest(oww_ctx* h, const void* in, int in_on_device, int32_t n_in, const uint8_t* stream_on, int stream_on_on_device,
                     float* scores, int scores_on_device);

/* ---- ingest classes: every stream its own rate and encoding in one launch ---------------------------------------------------------------
 * The serving example lets every connection announce its own sample rate and converts each message on the host
 * (examples/web/streaming_server.py:50-59); the entries above serve that only when all streams of a handle speak one format.  A
 * CLASS is what oww_ingest_configure takes -- (encoding, p, q, taps [q][n_taps], n_taps; n_taps = 0 with p = q = 1: decode only) -- a
 * handle holds a table of up to OWW_INGEST_MAX_CLASSES of them, and every stream belongs to one.  Per stream the arithmetic is that of
 * oww_ingest on a handle configured with the stream's class, bit for bit (same decode, same k-ordered fmaf chain over the padded row,
 * same rounding, same history).
 *   oww_ingest_configure_classes   after oww_commit; replaces any earlier ingest configuration (single or classes; per-class checks as
 *                       oww_ingest_configure, OWW_EINVAL naming the class).  Allocates one history int16 [S][Hpad], Hpad = the largest
 *                       class's n_taps - 1 rounded up to 8 (a stream uses the first n_taps - 1 of its own class; the rest stays zero),
 *                       the device table of class parameters, the padded banks back to back and the per-stream class id.  Every
 *                       stream starts in class 0 with a zero history; the state-record layout is rebuilt on demand.
 *   oww_ingest_assign   (examples/web/streaming_server.py:50-52: the connection's rate message) sets the class of the listed streams
 *                       and zeroes their histories: a caller arriving in a new format starts from silence.  Ordered on the handle's
 *                       stream like oww_reset, so it may follow submitted steps.  Unknown class, stream id out of range: OWW_EINVAL;
 *                       a handle without classes: OWW_ESTATE; nothing has moved then.
 *   oww_ingest_mixed    (examples/web/streaming_server.py:53-59: the per-message conversion) row s of `in` starts at s * row_bytes and
 *                       holds n_in(c) = n_out * p_c / q_c samples in the encoding of stream s's class c.  row_bytes: a multiple of 16
 *                       and at least the largest configured class's n_in * bytes per sample.  OWW_EINVAL, before any history moves,
 *                       when n_out * p_c is no multiple of q_c for a configured class or when a class's history + message exceed
 *                       the kernel's 96 KB of LDS staging.  out, stream_on: as oww_ingest (out == NULL: the staging buffer of
 *                       oww_ingest_dev).
 *   oww_step_ingest_mixed   oww_ingest_mixed into the staging buffer, then oww_step (n_out / 1280 chunks) or oww_step_masked (one
 *                       chunk), with every check of oww_step_ingest made before anything moves.
 *   oww_submit_ingest_mixed (examples/web/streaming_server.py:53-59 in the pipelined form of oww_submit_masked) one masked chunk,
 *                       n_out = 1280, stream_on == NULL: every stream.  in_host [S][row_bytes] goes up on the upload stream into the
 *                       slot's own device buffer; the compute stream waits for it, runs the mixed ingest into the staging buffer and
 *                       then the step; scores (and events) come down as after oww_submit; pair it with oww_collect.  in_host must
 *                       stay unmodified until that oww_collect; two steps in flight at most (OWW_ESTATE).
 * State: oww_reset zeroes the history of the streams it resets and KEEPS their class; oww_move_streams, oww_state_export and
 * oww_state_import carry history and class: the record's ingest part is Hpad / 2 words plus one 16-byte piece with the class id.
 * The fingerprint covers the whole table and every bank, so a record is refused by a handle with another table.  oww_ingest and
 * oww_step_ingest on a handle configured with classes, and the entries here on a handle configured with oww_ingest_configure, are
 * refused with OWW_ESTATE.  One launch serves all classes: its dynamic LDS is the largest class's need, which sets the occupancy for
 * every workgroup, and workgroups differ in work with their class.  Not counted by oww_kernel_times. */
#define OWW_INGEST_MAX_CLASSES 16
typedef struct oww_ingest_class {
    int32_t encoding;        /* OWW_ENC_* */
    int32_t p, q;            /* input rate / 16000 in lowest terms */
    int32_t n_taps;          /* even, <= 4096; 0 with p = q = 1: decode only */
    const float* taps;       /* [q][n_taps]; ignored when n_taps = 0 */
} oww_ingest_class;
int  oww_ingest_configure_classes(oww_ctx* h, int32_t n_classes, const oww_ingest_class* classes);
int  oww_ingest_assign(oww_ctx* h, const int32_t* stream_ids, int32_t n, const uint8_t* class_ids);
int  oww_ingest_mixed(oww_ctx* h, const void* in, int in_on_device, int64_t row_bytes, int32_t n_out, const uint8_t* stream_on,
                      int stream_on_on_device, int16_t* out, int out_on_device);
int  oww_step_ingest_mixed(oww_ctx* h, const void* in, int in_on_device, int64_t row_bytes, int32_t n_out, const uint8_t* stream_on,
                           int stream_on_on_device, float* scores, int scores_on_device);
int  oww_submit_ingest_mixed(oww_ctx* h, const void* in_host, int64_t row_bytes, const uint8_t* stream_on);

/* ---- head bank: each stream scored only by the wake-word models it subscribed to -----------------------------------------------------
 * openWakeWord's training pipeline (train.py, examples/custom_model.yml) yields one small binary head per phrase; a server that carries
 * many users' own phrases scores each connection with ITS heads, not with every head of the handle.  The embedding CNN (~94 % of a step)
 * is shared; the bank adds a device-resident set of heads, a per-stream subscription to up to K of them, and ONE routed heads launch per
 * hidden width (<= 64 and <= 128 units) that evaluates every (stream, subscribed head) pair once.
 *   oww_bank_configure  before oww_commit: K slots per stream (1..8) and the bank's capacity.  Allocates the subscription table [S][K]
 *                       (all slots empty), bank scores [S][K], score rings [S][K][30] and slot counters.  use_mfma = 3 only (OWW_ESTATE
 *                       otherwise).  A handle that never calls it allocates and launches nothing new.
 *   oww_bank_add        after commit, streams may be live: a head blob in the layout of oww_add_head -> bank id >= 0.  Accepted: kind 0
 *                       (binary sigmoid, n_out = 1), ungated, extra_blocks = 0, hidden <= 128, with or without LayerNorm, T <= the handle's
 *                       feature ring; anything else OWW_EINVAL naming the reason (such heads stay available as fixed heads).  The head
 *                       is packed like a fixed net of its width and self-tested on windows of oww_commit's probe embeddings against a
 *                       float64 evaluation: beyond 1e-3 it is refused with OWW_ERANGE, as oww_commit refuses weights.  A full bank:
 *                       OWW_EINVAL.
 *   oww_bank_remove     the slots subscribed to `id` become empty.
 *   oww_bank_set_postproc  patience / threshold of one bank head (model.py:340-359; patience <= 0 off, threshold NaN = none); the
 *                       debounce frames are the handle's (oww_set_postproc).  Default: off.
 *   oww_subscribe       bank_ids[n][K] for streams stream_ids[n]; -1 = empty slot.  A slot whose head changes restarts its prediction
 *                       count and ring (that model newly loaded into the stream's Model); the stream's audio, mel and feature state is
 *                       untouched.  oww_reset restarts the bank rings and counters of the streams it resets and keeps the subscriptions
 *                       (model.py:226-230).  Unknown ids or stream ids out of range: OWW_EINVAL, nothing changed.
 *   oww_bank_scores     syncs and copies the post-processed bank scores, host fp32 [S][K] (empty slot: 0.0); oww_bank_scores_dev: the
 *                       same on the device, valid until the next step.  They are the scores of the last step ENQUEUED on the handle: after oww_step /
 *                       oww_step_masked that call; with oww_submit, the newest submitted step (the call waits for it), which is the one
 *                       the last oww_collect delivered only while nothing else is in flight -- at two steps in flight collect both,
 *                       or read the bank scores of a step before submitting the next.
 *   oww_bank_routing    info = {tiles, waves per tile, entries} of the <= 64-unit launch, then of the <= 128-unit launch;
 *                       weight_bytes = first-layer weight bytes one step streams.
 * Semantics per (stream, slot): the raw score is the head's sigmoid output on the stream's last T feature rows (max over the chunks of a
 * multi-chunk call), bit for bit what the same net scores as a fixed head; then model.py:330-381 with the slot's own prediction count
 * (first-5 zeroing), the head's patience / threshold, a 30-deep ring per slot and the stream's VAD gate.  Masked steps leave every bit of a
 * sitting-out stream's bank state alone.  Every subscription or bank change re-captures the oww_use_graph graph on the next step.
 * Cost model: one workgroup per tile (1 or 4 waves = 32 or 128 entries of one head, chosen from the mean group size; largest tiles
 * first) streams that head's first-layer weights (T x 96 x 64 or 128 units, as f16 hi / lo halves: 0.39 / 0.79 MB at T = 16) once and
 * gathers each listed stream's ring rows (T x 384 bytes), so a step reads ~ tiles x weight bytes + entries x 6 KB.  Launches are counted
 * under kernel class 6 (heads) and the bank's post-processing under class 7; a bank without subscribers launches nothing. */
int  oww_bank_configure(oww_ctx* h, int32_t slots, int32_t capacity);
int  oww_bank_add(oww_ctx* h, const void* blob, size_t nbytes);
int  oww_bank_remove(oww_ctx* h, int32_t id);
int  oww_bank_set_postproc(oww_ctx* h, int32_t id, int32_t patience, float threshold);
int  oww_subscribe(oww_ctx* h, const int32_t* stream_ids, int32_t n, const int32_t* bank_ids);
int  oww_bank_scores(oww_ctx* h, float* out);
const float* oww_bank_scores_dev(const oww_ctx* h);
int  oww_bank_routing(oww_ctx* h, int32_t info[6], double* weight_bytes);

/* ---- per-stream custom verifiers: each stream re-scored by ITS user's verifier ------------------------------------------------------
 * custom_verifier_model.train_custom_verifier (custom_verifier_model.py:116-177) fits a verifier to one user's voice, and Model attaches
 * it to that user's Model (model.py:44-45, 185-195), with that Model's threshold.  oww_set_verifier above sets one verifier per label for
 * every stream of the handle; these entries assign verifiers per (stream, fixed score column) and per (stream, bank slot).
 *   oww_verifier_configure  before oww_commit: a device pool of `capacity` folded verifiers (1..65536; each w[T * 96] and a bias, T <= the
 *                       feature ring) and an assignment table of every (stream, fixed column) and (stream, bank slot) pair -- a verifier
 *                       id and a threshold each, all OWW_VERIFIER_DEFAULT.  A handle that never calls it allocates and launches exactly
 *                       what it did before.
 *   oww_verifier_add    after commit: the folded verifier of oww_set_verifier (w = coef / scale, n_w = T * 96, bias) -> pool id >= 0.
 *                       n_w not a multiple of 96, T beyond the ring or non-finite values: OWW_EINVAL; a full pool: OWW_EINVAL.
 *   oww_verifier_remove every assignment that names `id` reverts to OWW_VERIFIER_DEFAULT; the id is free again.
 *   oww_assign_verifiers       score column `label`, streams stream_ids[n]: verifier_ids[n], thresholds[n] (host pointers).
 *   oww_bank_assign_verifiers  the same for bank slot `slot`.
 *                       Ids: >= 0 a pool verifier; OWW_VERIFIER_DEFAULT the label's handle-wide oww_set_verifier setting, if any (a bank
 *                       slot has none: no verifier); OWW_VERIFIER_NONE no verifier, even where the label has a handle-wide one.  An
 *                       unknown id, a stream out of range, a pool verifier whose T differs from the T of the column's model or of the
 *                       slot's subscribed head, or a pool verifier for an empty slot: OWW_EINVAL, nothing changed.
 *   oww_verifier_stats  out = {pairs whose assignment is not OWW_VERIFIER_DEFAULT, verifier evaluations of the last step}; the second is
 *                       counted by the per-stream kernel only (0 while no pair is assigned and oww_set_verifier's kernel serves the label).
 *                       "The last step" is the newest one enqueued (the call waits for the handle's stream): with submitted steps in
 *                       flight that is the newest submitted step, not the one the last oww_collect delivered.
 * Semantics per (stream, column) and (stream, slot), one verification per call: the raw head output (max over the chunks of a multi-chunk
 * call); where it is >= the threshold it is replaced by sigmoid(w . last-T-feature-rows + bias) on the newest rows, bit for bit what
 * oww_set_verifier's path computes for the same (w, bias, threshold); then first-5 zeroing, patience / threshold / debounce, the 30-deep
 * ring (which keeps the verified score) and the VAD gate.  A per-stream assignment overrides the label's handle-wide verifier for that
 * stream.  oww_reset keeps assignments (Model.reset keeps custom_verifier_models); a bank slot whose head changes (oww_subscribe,
 * oww_bank_remove) drops its assignment back to the default; masked steps leave sitting-out streams alone; assignment calls wait for
 * queued steps (oww_submit) and re-capture the oww_use_graph graph on the next step.
 * Cost model: while any pair is assigned, one launch verifies every pair that has a verifier (a pool one or the handle-wide one), 16 pairs
 * per wave: a 16-byte list entry and the raw score per pair, then T x 96 x 4 bytes of feature rows and of weights per re-scored pair;
 * oww_set_verifier's kernel does not run then, and post-processing does not ride in the heads launch. */
#define OWW_VERIFIER_DEFAULT -1
#define OWW_VERIFIER_NONE    -2
int  oww_verifier_configure(oww_ctx* h, int32_t capacity);
int  oww_verifier_add(oww_ctx* h, const float* w, int32_t n_w, float bias);
int  oww_verifier_remove(oww_ctx* h, int32_t id);
int  oww_assign_verifiers(oww_ctx* h, int32_t label, const int32_t* stream_ids, int32_t n, const int32_t* verifier_ids, const float* thresholds);
int  oww_bank_assign_verifiers(oww_ctx* h, int32_t slot, const int32_t* stream_ids, int32_t n, const int32_t* verifier_ids, const float* thresholds);
int  oww_verifier_stats(oww_ctx* h, int64_t out[2]);

/* ---- fitting custom verifiers on the device (custom_verifier_model.py:95-113) ------------------------------------------------------
 * custom_verifier_model.train_verifier_model (custom_verifier_model.py:95-113) fits flatten -> StandardScaler ->
 * LogisticRegression(C = 0.001) to one user's feature windows.  oww_verifier_fit fits U such problems in one call and leaves each
 * result in the pool, folded, as oww_verifier_add would have: for problem u, windows offsets[u] .. offsets[u + 1] - 1 of `windows`
 * ([offsets[U]][T][96] fp32; a window flattened row-major as flatten_features does; on the device when windows_on_device, e.g.
 * oww_event_features_dev or the `windows` buffer of a hit list) with labels[i] in {0, 1} (host):
 *   mu, s = column mean and standard deviation (ddof = 0; s = 1 where a column is exactly constant), z = (x - mu) / s;
 *   (w~, b) = argmin C sum_i logloss(y_i, z_i . w~ + b) + 1/2 |w~|^2 (the intercept not penalised: scikit-learn's objective);
 *   w = w~ / s, bias = b - sum_j w_j mu_j  -> pool slot out[u].id, T recorded.
 * It is the optimum of that objective, not scikit-learn's iterate at its default tol = 1e-4, which sits up to 1e-3 in score from it.
 * Solved in the dual (an N x N Gram matrix per problem on f16-split MFMAs, then a Newton iteration in one workgroup); N = 2 ..
 * OWW_FIT_MAX_N windows per problem.  A problem's result does not depend on what else is in the call.
 * Per problem out[u].status: OWW_FIT_OK (id >= 0: the verifier is live in the pool); OWW_FIT_ONE_CLASS (scikit-learn raises there);
 * OWW_FIT_BAD_N (N < 2 or > OWW_FIT_MAX_N); OWW_FIT_NONFINITE (a window holds a NaN or an infinity); OWW_FIT_NOT_CONVERGED (the
 * iteration cap was reached).  Every status but OK gives id = -1, and the other problems of the call proceed.  iterations = Newton
 * steps, residual = max_i |a_i + C (p_i - y_i)| / C, the stationarity residual in score units.
 * Whole-call refusals (nothing changed): no pool or handle not committed (OWW_ESTATE); T outside 1 .. feature ring, offsets not
 * ascending, a label other than 0 or 1, C not finite or <= 0, fewer free pool slots than problems that pass the host-side checks
 * (OWW_EINVAL).  The work is enqueued on the handle's stream behind every submitted step and the call returns when it is done; the
 * step path of a handle that never calls it is unchanged.
 *   oww_verifier_get    reads pool verifier `id` back: w[n_w] (n_w = its T x 96) and *bias; waits for the handle's stream. */
#define OWW_FIT_MAX_N          1024
#define OWW_FIT_OK             0
#define OWW_FIT_ONE_CLASS      1
#define OWW_FIT_BAD_N          2
#define OWW_FIT_NONFINITE      3
#define OWW_FIT_NOT_CONVERGED  4
typedef struct { int32_t status, id, n_pos, n_neg, iterations; float residual; } oww_fit_result;
int  oww_verifier_fit(oww_ctx* h, const float* windows, int windows_on_device, const int64_t* offsets, const uint8_t* labels,
                      int32_t U, int32_t T, float C, oww_fit_result* out);      /* custom_verifier_model.py:95-113 */
int  oww_verifier_get(oww_ctx* h, int32_t id, float* w, int32_t n_w, float* bias);      /* custom_verifier_model.py:95-113: the fitted (coef / scale, folded intercept) */

/* ---- training bank heads on the device (train.py:434-510) ---------------------------------------------------------------------------
 * One step of train.Model.train_model for the network a bank head is (train.py:66-83 with n_blocks = 1, n_classes = 1: Linear ->
 * LayerNorm -> ReLU -> Linear -> LayerNorm -> ReLU -> Linear -> Sigmoid), U independent problems side by side, each with its own
 * parameters, Adam moments and counters, all drawing their batches from one pool of feature windows.  One session per handle.
 * The flat parameter record of a problem, oww_train_param_count(T, hidden) floats, holds the bank head's own fields in its order
 * and orientation (D = hidden):  w1 [96 T][D] | b1 [D] | ln1 gamma [D] | ln1 beta [D] | w2 [D][D] | b2 [D] | ln2 gamma [D] |
 * ln2 beta [D] | w3 [D] | b3 [1]   (w[in][out], as a head dict's "net" carries them).
 *   oww_train_begin     opens a session: U problems (1 .. 65535), T feature rows (1 .. the handle's feature ring), hidden a multiple
 *                       of 16 in 16 .. 128, params [U][oww_train_param_count] the initial records.  Moments start at zero, the
 *                       accumulation counters at (steps 1, samples 0), as train.py:443-444.
 *   oww_train_set_pool  the window pool [P][T][96] fp32, host memory or (pool_on_device) device memory; copied.
 *   oww_train_steps     K steps (1 .. OWW_TRAIN_MAX_STEPS) of n_batch slots (1 .. OWW_TRAIN_MAX_BATCH) for every problem, enqueued back
 *                       to back on the handle's stream behind every submitted step; returns when they are done.  idx / y are
 *                       [U][K][n_batch] (or [K][n_batch] with shared_tables, one table for all problems), host memory or
 *                       (tables_on_device) device memory: idx a pool row or -1 for an empty slot, y in {0, 1}.  Step k of the call,
 *                       per problem (train.py:447-510): forward; keep a sample iff (y = 0 and p >= 0.001) or (y = 1 and p < 0.999), m
 *                       kept; m = 0: nothing happens.  Otherwise acc_samples += m, and while acc_samples < 128: acc_steps += 1, no
 *                       update (the samples' gradients are dropped, as in the reference); else loss = (sum_kept w bce / m) /
 *                       acc_steps with w = neg_weight[k] for y = 0 and 1 for y = 1, one torch.optim.Adam step (betas 0.9 / 0.999,
 *                       eps 1e-8, bias correction by the count of optimizer steps taken) at learning rate lr[k], then acc_steps = 1,
 *                       acc_samples = 0.  The gradient at the logit is binary_cross_entropy's and Sigmoid's in fp32:
 *                       (p - y) / max(p (1 - p), 1e-12) * w * p (1 - p), zero where p rounds to exactly 0 or 1.
 *                       out [U][K]: loss as history["loss"] has it (NaN where no optimizer step was taken) and m.
 *   oww_train_get       the current record of problem u (waits for the handle's stream).
 *   oww_train_end       closes the session and releases its memory.
 * A problem's parameters have the same bits alone or among any other problems, with pool and tables in host or device memory, and
 * in one call of K steps or several calls that add up to them.  Refusals leave the session as it was: no session, or a second
 * oww_train_begin (OWW_ESTATE); U, hidden, T, n_batch or K outside their ranges, an index >= P or < -1, a label above 1, a
 * non-finite or negative lr or neg_weight (OWW_EINVAL).  A handle that never trains launches exactly what it did. */
#define OWW_TRAIN_MAX_BATCH 4096
#define OWW_TRAIN_MAX_STEPS 4096
typedef struct { float loss; int32_t m; } oww_train_record;
int64_t oww_train_param_count(int32_t T, int32_t hidden);      /* 0 for a form oww_train_begin refuses */
int  oww_train_begin(oww_ctx* h, int32_t U, int32_t T, int32_t hidden, const float* params);      /* train.py:66-83, 443-444 */
int  oww_train_set_pool(oww_ctx* h, const float* pool, int pool_on_device, int64_t P);
int  oww_train_steps(oww_ctx* h, int32_t K, int32_t n_batch, const int32_t* idx, const uint8_t* y, int shared_tables, int tables_on_device,
                     const double* lr, const float* neg_weight, oww_train_record* out);      /* train.py:447-510 */
int  oww_train_get(oww_ctx* h, int32_t u, float* params, int64_t n_params);
int  oww_train_end(oww_ctx* h);

/* ---- validating, checkpointing and merging the heads of a session (train.py:261-366) --------------------------------------------------
 * What Model.auto_train does around the step, for all problems of the open session at once, in the step's exact fp32 arithmetic; the
 * policy (when to validate, which checkpoint to keep, which to merge) stays with the caller (openwakeword_amd/train.py: auto_train).
 *   oww_train_new_sequence   a new train_model call on the same optimizer: for every problem acc_steps = 1, acc_samples = 0
 *                            (train.py:443-444); moments, the optimizer's step count and the parameters stay (train.py:135).
 *   oww_train_set_eval_pool  a second window pool [P][T][96] fp32 for validation, independent of the training pool; copied.
 *                            A pool larger than any before is allocated before the old one is released, so a refusal
 *                            (OWW_ENOMEM) leaves the old pool in use.
 *   oww_train_eval           the forward pass of train.py:66-83 for every problem over n slots (1 .. OWW_TRAIN_EVAL_MAX_ROWS) of the
 *                            eval pool, in the operation order of the training step's forward.  idx / y are [U][n] (or [n] with
 *                            shared_tables), host or (tables_on_device) device memory, idx an eval-pool row or -1 for an empty slot,
 *                            y in {0, 1}.  source = -1 reads the live parameters, 0 .. C - 1 a checkpoint slot.  counts [U]: n_pos,
 *                            n_neg, pos_gt (y = 1 and p > 0.5), neg_gt (y = 0 and p > 0.5), neg_ge (y = 0 and p >= 0.5), from which
 *                            the reference's metrics follow: self.fp (train.py:100, y - p <= -0.5) = neg_ge; binary Recall = pos_gt /
 *                            n_pos; binary Accuracy = (pos_gt + n_neg - neg_gt) / (n_pos + n_neg) (train.py:101-102, 544-553).
 *                            scores, if not null: [U][n] fp32 on the host, NaN in empty slots.  Runs behind every submitted step.
 *   oww_train_checkpoints    reserves C parameter slots (1 .. 65535) per problem, zero-filled; a second call replaces them.  Nothing
 *                            is allocated before this call; oww_train_end releases them.
 *   oww_train_snapshot       slot [U]: problem u's live parameters are copied to its slot slot[u] (-1: none), in stream order behind
 *                            the steps submitted before it (train.py:561, copy.deepcopy(self.model)).
 *   oww_train_average        sel [U][C] uint8.  A problem with at least one selected slot: slot dst receives average_models' result
 *                            (train.py:198-223) in its arithmetic: fp32, 0 * (the first selected slot), += every selected slot in slot
 *                            order, one division by their count.  A problem with none: dst receives its live parameters
 *                            (train.py:340-343).  dst may be among the selected.
 *   oww_train_get_slot       oww_train_get for checkpoint slot `slot` of problem u.
 * Counts are integers (integer atomics); a problem's scores and counts do not depend on what else is in the call, on where the
 * tables live, or on how a table is cut into calls.  Refusals leave the session as it was: no session, no eval pool or no slots
 * (OWW_ESTATE); a slot, source or n out of range, an index >= P or < -1, a label above 1 (OWW_EINVAL); slots whose size overflows 64
 * bits (OWW_EINVAL) or that cannot be allocated (OWW_ENOMEM).  A session that calls none of these allocates and launches what it did. */
#define OWW_TRAIN_EVAL_MAX_ROWS 1048576
typedef struct { int32_t n_pos, n_neg, pos_gt, neg_gt, neg_ge; } oww_train_counts;
int  oww_train_new_sequence(oww_ctx* h);      /* train.py:443-444 against train.py:135 */
int  oww_train_set_eval_pool(oww_ctx* h, const float* pool, int pool_on_device, int64_t P);
int  oww_train_eval(oww_ctx* h, int32_t source, int32_t n, const int32_t* idx, const uint8_t* y, int shared_tables, int tables_on_device,
                    float* scores, oww_train_counts* counts);      /* train.py:512-553 */
int  oww_train_checkpoints(oww_ctx* h, int32_t C);
int  oww_train_snapshot(oww_ctx* h, const int32_t* slot);      /* train.py:557-567 */
int  oww_train_average(oww_ctx* h, const uint8_t* sel, int32_t dst);      /* train.py:198-223, 326-343 */
int  oww_train_get_slot(oww_ctx* h, int32_t u, int32_t slot, float* params, int64_t n_params);

/* ---- stream state records: take a live stream's state out, put it in, move it ---------------------------------------------------------
 * In the reference a stream's state IS its Model object (prediction_buffer model.py:198, reset model.py:226-230; the AudioFeatures
 * buffers utils.py:163-171): a caller keeps it, hands it to another thread or pickles it.  Here that state lives in HBM in layouts only
 * the step kernels understand; these entries make it a portable record, so that a server can defragment its slots, drain a worker or
 * hand a connection to another handle without dropping the stream's context.  A stream that was exported and imported, or moved,
 * continues BIT FOR BIT as if it had stayed: scores do not depend on the slot or on the neighbours.
 *   oww_state_info    *record_bytes = size of one record (a multiple of 16), *fingerprint = 64-bit hash of what a record's bits depend
 *                     on: kernel family and interleave flag, per-layer history lengths, feature ring rows, score columns, bank slots,
 *                     VAD present or not, the 21 scale exponents of oww_calibration_info, and the bytes of every blob loaded (mel,
 *                     embedding, heads in order, VAD).  Either pointer may be NULL.
 *   oww_state_export  records of streams stream_ids[n], back to back in list order, into `out` (n * record_bytes; host, or a 16-byte
 *                     aligned device pointer when out_on_device).  Record = 32-byte header {magic, record layout version, record_bytes,
 *                     0, fingerprint, 0} + the stream's own words of every per-stream array that outlives a step, as bits, in a
 *                     slot-independent order: conv histories (for a grouped array: the words of the group block whose position is the
 *                     stream's, in ascending block index), PCM tail, feature ring and frame counter, score ring, prediction counter,
 *                     raw and final scores, VAD ring / counter and, with oww_load_vad, (h, c) and the last VAD score; with a bank, the
 *                     slots' raw / final scores, rings and counters.  Not carried: what one call writes and consumes (stage hand-over
 *                     buffers, mel rows, embeddings -- oww_get_mel is undefined after an import until the next step), the handle's
 *                     sticky range flag, subscriptions and verifier assignments (see oww_move_streams).
 *   oww_state_import  the reverse, into streams stream_ids[n] (no duplicates).  Every header is checked first: a record of another
 *                     layout version, record size or fingerprint, a duplicate or out-of-range id -> OWW_EINVAL (the message names
 *                     both sides) and the handle is untouched.  Writes only the words the target streams own: the other streams of
 *                     a shared group block keep every bit.  Subscriptions and verifier assignments are the caller's business on the
 *                     target handle: oww_subscribe first (which restarts the slot), then import (which puts ring and counter back).
 *   oww_move_streams  export + import inside one handle without the host: stream src[i] becomes stream dst[i].  All reads happen
 *                     before any write, so swaps, cycles and chains (a->b, b->c) are legal; dst holds no duplicates.  The device state
 *                     of a source that is nobody's destination keeps its contents (reset it when the slot is reused).  What the
 *                     LIBRARY keeps per stream travels too: bank subscriptions and per-stream verifier assignments (fixed columns and
 *                     bank slots) leave the source slot -- a source that is nobody's destination ends up with empty slots and default
 *                     assignments -- and arrive at the destination; a moved bank slot does NOT restart.  The routing table and the
 *                     verifier list are rebuilt once per call, and only then is the oww_use_graph graph re-captured on the next step.
 * All four return OWW_ESTATE before oww_commit.  Export, import and move run on the handle's stream behind every queued step
 * (oww_submit) and return when they are complete.  A handle that never calls them allocates and launches exactly what it did before;
 * the first call builds the layout table and hashes the weights (a few ms).
 * Cost model: pure data movement, ~50 KB per stream and direction.  One launch per array kind, work per (stream, array): 16-byte
 * accesses on the record side always and on the live side for every array in which a stream's words are contiguous.  The deeper conv
 * histories interleave 2 / 4 / 8 streams (VAD: 16) in every 64-byte run, so a lone stream touches its whole group block there (about
 * 4x its own bytes over the record); a list that names every stream of a block is served as full rows, at the cost of a plain copy.
 * These launches are not counted by oww_kernel_times. */
int  oww_state_info(oww_ctx* h, size_t* record_bytes, uint64_t* fingerprint);
int  oww_state_export(oww_ctx* h, const int32_t* stream_ids, int32_t n, void* out, int out_on_device);
int  oww_state_import(oww_ctx* h, const int32_t* stream_ids, int32_t n, const void* in, int in_on_device);
int  oww_move_streams(oww_ctx* h, const int32_t* src, const int32_t* dst, int32_t n);

/* ---- detection events: the hits of a call as ordered device-side records, with the feature window the head saw ---------------------
 * A caller of oww_step otherwise copies [S][n_labels] (and [S][K] bank) scores back and scans them for score >= threshold, and the
 * evidence of a detection -- the feature rows behind it, for a second-stage verifier, a log or custom-verifier training (the reference:
 * examples/capture_activations.py, Model._get_positive_prediction_frames model.py:428-476) -- is gone from the ring by the time a
 * pipelined caller sees the score.  With events configured, two small launches behind every step compact the hits into records and
 * copy each hit's last feature rows in the step that detected.
 *   oww_events_configure  before oww_commit: room for `capacity` events per call (1 .. 1<<20) and `feature_rows` snapshot rows per event
 *                       (0 = none .. the handle's feature ring; a value beyond the ring, which is only known once every head is loaded,
 *                       makes oww_commit return OWW_EINVAL).  Allocates capacity x (32 + feature_rows x 384) bytes on the device, and
 *                       again per pipeline slot at the first oww_submit.  Every pipelined step (oww_submit) then brings the slot's whole
 *                       record buffer, capacity x 32 bytes, to page-locked host memory behind its scores WHATEVER the hit count (the
 *                       count is not known to the host when the copy is queued): 128 KB at capacity 4,096, 32 MB at 1 << 20 -- size the
 *                       capacity to the hits one call can have, not to the limit.  A handle that never calls it allocates and launches
 *                       exactly what it did before, and the other entries return OWW_ESTATE.
 *   oww_events_set_thresholds  after commit: fixed[n_labels] event thresholds of the score columns (NULL = keep) and the one of every
 *                       bank slot (NaN = keep).  Default 0.5 everywhere; a NaN column threshold = the column never reports.
 *   oww_get_events      up to `cap` records of the last call into `out` (host), *n_stored = records the call stored = min(*n_total,
 *                       capacity), *n_total = hits the call had; n_stored < n_total is the overflow signal, not an error.  Any of the
 *                       three pointers may be NULL.  Which call: after oww_step / oww_step_masked that call (waits for the handle's
 *                       stream); after oww_collect the collected step, whose counts and records came to page-locked host memory behind
 *                       its scores (a memcpy, whatever is in flight by then).  Valid until the next step or submit; before any call,
 *                       and between a submit and the next collect: zero events.
 *   oww_get_event_features  snapshots of records [first, first + n) of that same call: fp32 [n][feature_rows][96], oldest row first --
 *                       bit for bit what oww_get_features(stream, feature_rows) read right after the detecting step.  Host pointer, or a
 *                       16-byte aligned device pointer with out_on_device.  Snapshots stay on the device until asked for; the copy runs
 *                       on the handle's stream (behind a step that is in flight).  first + n beyond n_stored, or feature_rows == 0:
 *                       OWW_EINVAL.
 *   oww_events_dev      device records of the last synchronous call (oww_step / oww_step_masked), *count_dev = device {n_stored,
 *                       n_total}; valid until the next step; for consumers on the device (enqueue behind the step on the handle's
 *                       stream).  oww_event_features_dev: the snapshots of the same call, [capacity][feature_rows][96] (NULL with
 *                       feature_rows == 0): the supported way for a second-stage verifier on the device to read the windows of
 *                       records [0, n_stored) without the copy of oww_get_event_features.  Both buffers hold one spare record /
 *                       snapshot behind index capacity - 1 that the library never writes.
 * Hit: a (stream, fixed score column) or (stream, bank slot with a subscription) pair whose stream took part in the call and whose
 * post-processed score -- after verifier, patience / debounce and VAD gate: bit for bit what oww_step returns or oww_bank_scores reads
 * -- is >= its event threshold.  A stream that sits a masked step out reports nothing although its score row repeats; a multi-chunk or
 * long call reports once, with the call's score; debounce_frames gives one event per utterance.
 * Order: ascending stream; within a stream the fixed columns ascending, then the slots ascending.  The first min(n_total, capacity)
 * hits in that order are stored.  `frame` is the stream's prediction counter after the call (the number of calls the stream took part
 * in since its reset; a handle without fixed heads advances it too).
 * Cost model: 2 launches of ceil(S x (n_labels + K) / 256) workgroups, timed under kernel class 7; each reads the pairs' scores (4
 * bytes per pair, twice) and writes 32 + feature_rows x 384 bytes per stored hit.  Not part of the oww_use_graph graph. */
typedef struct oww_event {     /* 32 bytes */
    int32_t  stream;
    int32_t  column;           /* fixed head: score column >= 0; bank: ~slot (negative) */
    int32_t  bank_id;          /* subscribed bank id for a slot, -1 for a fixed column */
    float    score;            /* the post-processed score, bit for bit what oww_step returns */
    uint32_t frame;            /* the stream's prediction counter after this call */
    int32_t  feature_index;    /* index of this event's snapshot, -1 when feature_rows == 0 */
    int32_t  reserved[2];      /* 0 */
} oww_event;
int  oww_events_configure(oww_ctx* h, int32_t capacity, int32_t feature_rows);
int  oww_events_set_thresholds(oww_ctx* h, const float* fixed, float bank);
int  oww_get_events(oww_ctx* h, oww_event* out, int32_t cap, int32_t* n_stored, int32_t* n_total);
int  oww_get_event_features(oww_ctx* h, int32_t first, int32_t n, float* out, int out_on_device);
const oww_event* oww_events_dev(const oww_ctx* h, const int32_t** count_dev);
const float* oww_event_features_dev(const oww_ctx* h);

/* ---- audio: each stream's recent 16 kHz PCM on the device, and the audio behind every event -------------------------------------------
 * The reference keeps the last 10 s of a stream's audio beside its features (AudioFeatures.raw_data_buffer, utils.py:164,174,407), and its
 * tooling lives on that buffer: examples/capture_activations.py:134-174 writes the last 5 s to a WAV one second after an activation,
 * custom-verifier training clips are cut from it, and a deployment hands the command behind the wake word to a recogniser.  Here a
 * stream's audio otherwise lives for one step, and with the ingest entries (oww_step_ingest*, oww_submit_ingest_mixed) it never exists on
 * the host at all.  With audio configured the handle keeps a ring int16 [S][ring_chunks][1280] and one uint32 chunk counter per stream.
 *   oww_audio_configure  before oww_commit: ring_chunks 1 .. 1024 per stream (the reference's 10 s: 125) and event_chunks 0 ..
 *                       ring_chunks snapshot chunks per event (a positive value needs oww_events_configure: without it oww_commit
 *                       returns OWW_EINVAL).  oww_commit allocates S x ring_chunks x 2,560 bytes (64-bit arithmetic: 131,072 x 125
 *                       chunks are 42 GB) and, per event buffer set -- one for the synchronous calls, one per pipeline slot at the first
 *                       oww_submit -- (capacity + 1) x event_chunks x 2,560 bytes; what does not fit is OWW_ENOMEM, with the bytes in
 *                       the message.  A handle that never calls it allocates and launches exactly what it did before, produces the same
 *                       bits and reports the same oww_state_info; the read entries then return OWW_ESTATE, oww_event_audio_dev NULL.
 *   Append              every call that advances streams -- oww_step (multi-chunk and long calls: the whole call once),
 *                       oww_step_masked, oww_step_ingest, oww_step_ingest_mixed, oww_submit, oww_submit_masked, oww_submit_ingest_mixed
 *                       (from the slot's own buffer, on the compute stream) -- appends the call's 16 kHz samples exactly as the front end
 *                       consumed them (ingest: the decoded and resampled staging buffer) to the ring of every stream that took part:
 *                       its k chunks in order, of a call with k > ring_chunks the last ring_chunks, and k is added to the stream's
 *                       counter.  A stream that sits a masked step out keeps every bit of ring and counter.  The append runs behind
 *                       the step's launches and before the events, so a snapshot ends with the detecting chunk; it is not part of the
 *                       oww_use_graph graph, and oww_embed, oww_embed_clips, oww_mel and the commit probes never touch a ring.
 *                       oww_reset zeroes ring and counter of the streams it resets (utils.py:174).
 *   oww_get_audio       the newest n_chunks (1 .. ring_chunks) chunks of streams stream_ids[n] (duplicates and any order), oldest
 *                       first, as int16 [n][n_chunks * 1280] into `out` (host, or a 16-byte aligned device pointer with out_on_device);
 *                       chunks the stream has not received since its reset read as zero.  counts (host [n], or NULL): the streams'
 *                       counters.  Like oww_state_export it runs on the handle's stream behind every queued step and returns when it is
 *                       complete: with submitted steps in flight the rings and counters are those behind the NEWEST submitted step, not
 *                       behind the one the last oww_collect delivered (oww_get_event_audio is the per-step view).  This is the
 *                       post-roll path: for "one second after the hit" ask for the stream 13 steps later.
 *   oww_get_event_audio  snapshots of records [first, first + n) of the call oww_get_events refers to: int16 [n][event_chunks * 1280],
 *                       the newest event_chunks chunks of the record's stream in the detecting step, oldest first, zero where the
 *                       stream had received less since its reset.  Snapshot i belongs to stored record i (the rank, as with
 *                       feature_index).  Validity, host / device `out` and the wait as oww_get_event_features; pipelined steps keep
 *                       their snapshots in the slot's own device buffer until asked.  first + n beyond n_stored, or event_chunks == 0:
 *                       OWW_EINVAL.
 *   oww_event_audio_dev  the snapshots of the last synchronous call on the device, [capacity][event_chunks][1280], the counterpart of
 *                       oww_event_features_dev (NULL without event_chunks); one spare snapshot behind index capacity - 1 is never written.
 * State records: with audio a record gains two flat sections behind the others, the ring (ring_chunks x 2,560 bytes, as it lies) and a
 * 16-byte piece with the counter, and the fingerprint covers ring_chunks: a record from a handle with another ring is refused as any
 * other configuration mismatch.  oww_move_streams carries both; a moved or imported stream's later snapshots and oww_get_audio reads are
 * bit for bit those of a stream that stayed.
 * Every failing call leaves the handle untouched: out-of-range ring_chunks / event_chunks / n_chunks / stream id / record range ->
 * OWW_EINVAL, oww_audio_configure after commit -> OWW_ESTATE.
 * Cost model: pure data movement in 16-byte pieces, timed under kernel class 7.  Per stream and chunk the append reads 2,560 bytes and
 * writes 2,560 (one wave per stream, one launch per call: 0.67 GB per step at 131,072 streams); a snapshot launch, only with
 * event_chunks > 0, moves 2 x event_chunks x 2,560 bytes per stored event on a grid sized to the chip, not to the capacity;
 * oww_get_audio moves 2 x n_chunks x 2,560 bytes per listed stream plus the copy to the host and is not counted by oww_kernel_times. */
int  oww_audio_configure(oww_ctx* h, int32_t ring_chunks, int32_t event_chunks);
int  oww_get_audio(oww_ctx* h, const int32_t* stream_ids, int32_t n, int32_t n_chunks, int16_t* out, int out_on_device, uint32_t* counts);
int  oww_get_event_audio(oww_ctx* h, int32_t first, int32_t n, int16_t* out, int out_on_device);
const int16_t* oww_event_audio_dev(const oww_ctx* h);

/* ---- multi-GPU: delivery of the scores to one rank over RCCL (xGMI), for binders without torch.distributed ----------------------
 * Streams are independent, so N GPUs = N handles in N processes, each owning a contiguous range of the global streams (the
 * reference's only scale-out, utils.py:502-536 bulk_predict, splits FILES over processes the same way); nothing in the data path
 * crosses GPUs.  The one exchange is handing the per-stream scores to whoever consumes them:
 *   oww_comm_id       rank 0: fills id[OWW_COMM_ID_BYTES] (ncclGetUniqueId); the binder ships these bytes to the other ranks by
 *                     whatever side channel it has (a file, a socket, an environment variable, MPI)
 *   oww_comm_init     every rank, collectively: joins the communicator (ncclCommInitRank) on the handle's device
 *   oww_gather_scores enqueued on the handle's stream after a step: every rank sends its fp32 [S_r][n_labels] scores to rank 0,
 *                     which receives them at out + sum(counts[0..r)) * n_labels (device pointer; counts[r] = streams of rank r, the
 *                     same array on every rank).  One grouped ncclSend / ncclRecv exchange; asynchronous (oww_sync to wait).
 *   oww_comm_count    *ranks = what the communicator itself reports (ncclCommCount): the number of RCCL ranks actually joined
 *   oww_comm_destroy  leaves the communicator (oww_destroy does it too)
 * librccl.so is bound at run time by the first of these calls; a process that already holds a copy (e.g. torch's) shares it.
 * Python: openwakeword_amd.shard.ScoreGather is the torch.distributed form of the same exchange. */
#define OWW_COMM_ID_BYTES 128
int  oww_comm_id(void* id);
int  oww_comm_init(oww_ctx* h, const void* id, int32_t rank, int32_t world);
int  oww_gather_scores(oww_ctx* h, float* out, const int32_t* counts);
int  oww_comm_count(oww_ctx* h, int32_t* ranks);
int  oww_comm_destroy(oww_ctx* h);

/* ---- stage-level entry points (the reference's per-stage closures; used for parity tests and for
 *      AudioFeatures._get_melspectrogram / embed_clips style callers).  Host pointers. ---------------
 * oww_mel: int16 [B][n] -> dB values [B][F][32], F=(n-512)/160+1, clamp floor shared over the call
 *          exactly like melspec_model_predict (utils.py:87,202).  Requires B <= n_streams.
 * oww_embed: mel rows [B][rows][32] (rows = 76 + 8*(n_out-1)) -> embeddings [B][n_out][96]; the
 *          windows are rows[8i : 8i+76] (utils.py:229-236).  Runs the same incremental kernels; the
 *          streaming state of the streams it borrows is parked and put back, so live streams are unaffected.
 * oww_head: features [B][T][96] -> raw outputs [B][n_out] of head `head` (model.py:137-138). */
int  oww_mel(oww_ctx* h, const int16_t* pcm, int32_t B, int32_t n, float* out_db);
/* the same with one clamp floor PER CLIP: what the reference's CPU path computes when it maps _get_melspectrogram over
 * the clips of a batch (utils.py:243-290, embed_clips / feature extraction for training, utils.py:542-601) */
int  oww_mel_clips(oww_ctx* h, const int16_t* pcm, int32_t B, int32_t n, float* out_db);
int  oww_embed(oww_ctx* h, const float* mel_rows, int32_t B, int32_t rows, float* out);
/* AudioFeatures.embed_clips (utils.py:354-385; the feature extractor behind compute_features_from_generator,
 * utils.py:542-601): int16 clips [B][n] -> embeddings [B][n_out][96], n_out = (F-76)/8 + 1 with F = (n-512)/160 + 1
 * mel frames per clip.  Everything stays on the device: per-clip mel (one clamp floor per clip, x/10+2), then the
 * incremental CNN walks each clip in steps of 8 mel rows (4 lead-in rows + 9 warm-up steps, then one embedding per
 * step) -- 7.5x fewer flops than evaluating every 76-row window on its own, same results.  `pcm` / `out` are host
 * pointers unless the matching *_on_device flag is set.  Requires B <= n_streams, F >= 76; like oww_embed it borrows the
 * streaming machinery of streams [0,B) and restores their state before returning. */
int  oww_embed_clips(oww_ctx* h, const int16_t* pcm, int32_t pcm_on_device, int32_t B, int32_t n,
                     float* out, int32_t out_on_device);
int  oww_head(oww_ctx* h, int32_t head, const float* features, int32_t B, float* out);

/* ---- dense scoring: every window of a feature sequence through the fixed heads -----------------------------------------------------
 * The reference scores recordings as well as live streams: train.py:874-879 slices hours of precomputed features [N][96] into every
 * T-row window (stride 1) and runs the head over all of them, Model._get_positive_prediction_frames (model.py:428-479, behind
 * examples/mine_false_positives.py) keeps the windows of long audio that score above a threshold, utils.bulk_predict
 * (utils.py:502-536) walks files chunk by chunk.  These entries score all windows of B sequences in one call.
 *   oww_score_shape     t_max = the largest T over the handle's fixed heads, n_win = n_rows - t_max + 1; either pointer may be NULL.
 *   oww_score_features  feats fp32 [B][n_rows][96] (host, or a 16-byte aligned device pointer with feats_on_device) ->
 *                       out fp32 [B][n_win][n_labels] (host or device).  Replaces train.py:874-879 and model.py:313-317 per window.
 *   oww_score_clips     int16 clips [B][n] -> the same scores over the clips' oww_embed_clips embeddings (n_rows = that entry's n_out),
 *                       which never leave the device; emb_out (may be NULL): the embeddings [B][n_out][96] exactly as
 *                       oww_embed_clips returns them (host, or device with emb_on_device).  Replaces model.py:428-479 and the
 *                       per-chunk loop of utils.py:502-536.
 * Window alignment: window w of sequence b ends at row w + t_max - 1, and a head of window length T reads rows
 * [w + t_max - T, w + t_max), its own last T rows -- what the heads of one live handle see at one instant.  Every entry of `out` is
 * defined.  n_rows < t_max: OWW_EINVAL.
 * Values: out[b][w][col] is the raw head output, what model_prediction_function returns (model.py:313-317); in the fp16-split family
 * (use_mfma = 3) and every other family it is bit for bit what oww_head returns for that head on the materialised window.  No first-5
 * zeroing, patience, debounce, verifier or VAD gate: those are properties of a live stream.  Fixed heads only -- bank heads are
 * scored by oww_bank_score_* below -- and a handle without fixed heads returns OWW_EINVAL.
 * Last window: train.py:875's range(0, N - T, 1) drops the last window; these entries return all n_rows - T + 1, and out[:, :-1] is
 * the reference's set.
 * Independence: a window's scores depend on its rows alone -- not on B, on the other sequences or on where the window falls in a
 * tile -- so a long array may be scored in chunks that overlap by t_max - 1 rows, with identical bits.
 * Live streams: oww_score_features borrows no stream state (streams, rings, events, audio rings and the captured graph are
 * untouched); oww_score_clips parks and restores streams [0, B) exactly as oww_embed_clips does (B <= n_streams, one mel clamp floor
 * per clip).
 * Paths: narrow fp16-split groups (<= 64 hidden units, 1-4 nets, gated pairs included: every released binary model) run the
 * sliding-window kernel (owwhip_dense.h) at every T, one launch per pass of one or two nets: it stages, scales and splits each feature
 * row once per tile of 256 windows (128 beyond T = 113 for one net, 72 for two) instead of once per window; every other head (wide
 * and generic nets, recurrent heads, use_mfma 0 / 1 / 2) has its windows gathered on the device into a slab of at most 256 MiB and
 * scored as oww_head scores them.
 * Errors and accounting: OWW_ESTATE before oww_commit; bad arguments OWW_EINVAL with the handle untouched; sizes in 64-bit
 * arithmetic, what does not fit is OWW_ENOMEM with the bytes in the message; the sticky range flag is raised and reported as by
 * oww_head (position unknown).  The heads launches are timed under kernel class 6, the fallback's window gather under class 7. */
int  oww_score_shape(oww_ctx* h, int32_t n_rows, int32_t* n_win, int32_t* t_max);
int  oww_score_features(oww_ctx* h, const float* feats, int feats_on_device, int32_t B, int32_t n_rows,
                        float* out, int out_on_device);
int  oww_score_clips(oww_ctx* h, const int16_t* pcm, int pcm_on_device, int32_t B, int32_t n,
                     float* out, int out_on_device, float* emb_out, int emb_on_device);

/* ---- dense scoring over the head bank: validate many heads on one corpus --------------------------------------------------------------
 * Before a newly trained head goes live its false-accept rate is checked on a negative corpus.  The reference does this for a list of
 * candidate models: train.py:225-258 (_select_best_model) runs every model of self.best_models over the false-positive validation
 * features, which train.py:874-879 slices into every T-row window, and train.py:100 counts the windows with pred >= 0.5 (divided by
 * the hours at train.py:513-522).  These entries score every window of B sequences with a LIST of bank heads in one call.
 *   oww_bank_score_shape     t_max = the largest T over the LISTED bank heads, n_win = n_rows - t_max + 1; either pointer may be NULL.
 *   oww_bank_score_features  feats fp32 [B][n_rows][96] (host, or a 16-byte aligned device pointer with feats_on_device) ->
 *                            out fp32 [B][n_win][n_ids] (host, or a 16-byte aligned device pointer): out[b][w][i] is the raw sigmoid
 *                            output of bank head bank_ids[i] on window w.
 *   oww_bank_score_stats     the same scores reduced on the device, inside the kernel that computes them; the matrix (1,024 heads x 8
 *                            hours: 1.5 GB) is never written.  Host arrays, each [B][n_ids]:
 *                              count[b][i]  = #{w : out[b][w][i] >= thresholds[i]}   (thresholds NULL = 0.5, train.py:100's default)
 *                              max[b][i]    = the maximum over w;   argmax[b][i] = the smallest w that attains it
 *                            bit for bit what numpy computes from the matrix, whatever the scheduling: integer atomics on a key
 *                            that orders like the score (a sigmoid output is >= +0) with the complement of w below it.
 * Window alignment: as oww_score_features with t_max taken over the listed heads -- window w ends at row w + t_max - 1 and head i of
 * length T_i reads rows [w + t_max - T_i, w + t_max).  Values: bit for bit what the same net scores as a fixed head through
 * oww_score_features; no first-5 zeroing, patience, verifier or VAD gate.  Duplicate ids give duplicate columns.  train.py:875 drops
 * the last window; these entries do not.
 * Live streams: the entries run on the handle's stream and read and write nothing of the live streams: subscriptions, bank raw
 * scores, scores and rings, the routing table, events and the captured graph are untouched.
 * Paths: the listed narrow heads (<= 64 hidden units) run as ONE launch of heads_dense_bank_kernel (owwhip_dense.h): grid = (sequence x
 * tile) x head slices, a workgroup stages its tile's rows once and walks the heads of its slice (OWW_DENSE_BANK_HPW overrides the
 * heads per workgroup: an A/B aid).  Wide heads (65-128 units) and everything with OWW_DENSE_PATH=ext take the fallback: window
 * gather into the bounded slab, heads_bank_kernel as oww_bank_add's self-test launches it, a small kernel from the slab's scores into
 * the column or the statistics -- the same bits.
 * Errors (nothing has moved): OWW_ESTATE before oww_commit or without a bank; OWW_EINVAL for n_ids < 1, an id that is not a live
 * bank head (named in the message), n_rows < t_max, a NaN threshold, a null or misaligned device pointer; sizes in 64-bit arithmetic,
 * what does not fit is OWW_ENOMEM with the bytes in the message.  The sticky range flag is raised and reported as by oww_head
 * (position unknown); when it is up, the statistics of that call are not defined.  Heads launches are timed under kernel class 6,
 * gathers and the fallback's scatter / reduction under class 7. */
int  oww_bank_score_shape(oww_ctx* h, const int32_t* bank_ids, int32_t n_ids, int32_t n_rows, int32_t* n_win, int32_t* t_max);
int  oww_bank_score_features(oww_ctx* h, const float* feats, int feats_on_device, int32_t B, int32_t n_rows,
                             const int32_t* bank_ids, int32_t n_ids, float* out, int out_on_device);
int  oww_bank_score_stats(oww_ctx* h, const float* feats, int feats_on_device, int32_t B, int32_t n_rows,
                          const int32_t* bank_ids, int32_t n_ids, const float* thresholds,
                          int32_t* count, float* max, int32_t* argmax);

/* ---- dense scoring: ordered hit lists with their feature windows ----------------------------------------------------------------------
 * Between the full matrix and three numbers per head lies what the reference's users mine: Model._get_positive_prediction_frames
 * (model.py:428-479, behind examples/mine_false_positives.py) returns, per label, the feature windows of every frame that scored at
 * least a threshold, and train.py feeds such windows back as hard negatives.  These entries return, per column, the positions, the
 * scores and the feature windows of the hits -- and nothing else: neither the matrix nor, in the clip entry, the embeddings leave the
 * device.
 *   Columns: n_cols = oww_n_labels() for oww_score_hits / oww_score_clip_hits, n_ids for oww_bank_score_hits (duplicate ids give
 *   duplicate columns).  A HIT is a (sequence, window, column) whose entry in the matrix of oww_score_features / oww_score_clips /
 *   oww_bank_score_features is >= thresholds[column]; thresholds NULL = 0.5 everywhere (train.py:100).  A fixed column with a NaN
 *   threshold never reports (as oww_events_set_thresholds); a NaN threshold of the bank entry is OWW_EINVAL (as oww_bank_score_stats).
 *   Window alignment, t_max, gating and multiclass columns are the matrix entries'; the test is applied to the value they would store.
 *   hits      host, [n_cols][cap]: column c receives its hits in ascending (seq, window) order, the first min(n_total[c], cap) of
 *             them, whatever the scheduling; n_stored[c] is that number, n_total[c] the number of hits the column had.  n_stored <
 *             n_total is the overflow signal, not an error; every column has its own cap slots.  score: bit for bit the matrix entry.
 *             Slots beyond n_stored[c] are not written.  cap is 1 .. 1 << 20.
 *   windows   NULL, a host pointer or a 16-byte aligned device pointer: stored hit i of column c has the head's own last T_c rows of
 *             its window, oldest first, as fp32 [T_c][96] at win_offset[c] + i * T_c * 96 floats -- bit for bit the rows of feats, or
 *             of the embeddings oww_embed_clips would return.  oww_score_hits_layout fills win_offset[n_cols + 1] (the last entry is
 *             the buffer's size in floats) for the fixed columns (bank_ids NULL) or a list of bank heads.
 *   n_total[c] = the sum over b of oww_bank_score_stats' count[b][c].  A call's results depend on a window's rows alone, so chunks of a
 *   long array that overlap by t_max - 1 rows concatenate to the whole array's list (up to cap).
 * How: the heads launches of the matrix entries run in a hit-mask mode -- one bit per (column, sequence, window), one plain 32-bit
 * store per wave and column (n_cols x B x ceil(n_win / 32) words: 32 MB for 1,024 heads at 2^18 rows) -- then one workgroup per column
 * compacts its words in order (popcount, scan, carry: no atomics), and only the stored hits' windows are gathered and re-scored as
 * external features by the kernels of the fallback path, whose bits are the sliding kernels'.  Cost model: the heads launches of the
 * matrix entry, + 1 / 32 word per window and column written and read once, + work proportional to n_cols x min(hits, cap).
 * Errors, live streams and accounting follow the matrix entries: OWW_ESTATE before oww_commit (or without a bank); OWW_EINVAL with
 * nothing moved for a cap outside 1 .. 1 << 20, null hits / n_stored / n_total, n_rows < t_max, a dead bank id, a misaligned device
 * pointer; 64-bit sizes and OWW_ENOMEM with the bytes in the message; nothing of the live streams moves, except that the clip entry
 * parks streams [0, B) as oww_embed_clips does; the range flag behaves as oww_head's.  Heads launches (the re-score included) are
 * timed under kernel class 6; mask compaction, gathers and slab passes under class 7. */
typedef struct oww_dense_hit { int32_t seq; int32_t window; float score; int32_t reserved; /* 0 */ } oww_dense_hit;   /* 16 bytes */
int  oww_score_hits_layout(oww_ctx* h, const int32_t* bank_ids, int32_t n_ids, int32_t cap, int64_t* win_offset);
int  oww_score_hits(oww_ctx* h, const float* feats, int feats_on_device, int32_t B, int32_t n_rows,
                    const float* thresholds, int32_t cap,
                    oww_dense_hit* hits, int32_t* n_stored, int64_t* n_total, float* windows, int windows_on_device);
int  oww_score_clip_hits(oww_ctx* h, const int16_t* pcm, int pcm_on_device, int32_t B, int32_t n,
                         const float* thresholds, int32_t cap,
                         oww_dense_hit* hits, int32_t* n_stored, int64_t* n_total, float* windows, int windows_on_device);
int  oww_bank_score_hits(oww_ctx* h, const float* feats, int feats_on_device, int32_t B, int32_t n_rows,
                         const int32_t* bank_ids, int32_t n_ids, const float* thresholds, int32_t cap,
                         oww_dense_hit* hits, int32_t* n_stored, int64_t* n_total, float* windows, int windows_on_device);

/* ---- introspection ------------------------------------------------------------------------------ */
/* AudioFeatures.get_features (utils.py:454-460): last T rows of stream sid's feature ring, oldest first.  Waits for the handle's
 * stream: the ring as the newest enqueued step left it -- with submitted steps in flight, the newest submitted one, not the one the
 * last oww_collect delivered (oww_get_raw and oww_get_mel likewise). */
int  oww_get_features(oww_ctx* h, int32_t sid, int32_t T, float* out);
/* newest n_rows (<= 8*n_chunks of the last step) transformed mel rows (x/10+2) of stream sid from the last step */
int  oww_get_mel(oww_ctx* h, int32_t sid, float* out, int32_t n_rows);
/* per-layer CNN outputs (new rows only, dense [rows][F][C]) of stream sid from the last chunk processed;
 * layer 0..19; needs cfg.debug_layers.  Returns the number of floats written. */
int  oww_debug_read(oww_ctx* h, int32_t sid, int32_t layer, float* out, int32_t cap);
/* in-kernel phase stamps (shader clock) of one workgroup of each of the four generic CNN stage kernels
 * from the last step: out[stage 0..3][wave 0..15][mark 0..15]; only when the environment variable
 * OWW_PROF_BLOCK=<workgroup index> was set at oww_commit time.  Development aid. */
int  oww_debug_profile(oww_ctx* h, int64_t* out, int32_t cap);
/* kernel timing: records hipEvents around every kernel of subsequent oww_step calls when enabled;
 * oww_kernel_times fills ms[i] with the accumulated time and n[i] with the launch count of kernel
 * class i (0 mel,1 stageA,2 stageB,3 stageC,4 stageD,5 stageE,6 heads,7 postproc,8 vad_front,9 vad_lstm) and clears them. */
#define OWW_N_KERNEL_CLASSES 10
int  oww_enable_timing(oww_ctx* h, int on);
int  oww_kernel_times(oww_ctx* h, double ms[OWW_N_KERNEL_CLASSES], int64_t n[OWW_N_KERNEL_CLASSES]);
/* capture the n_chunks==1 device-to-device step into a hipGraph and replay it on later steps */
int  oww_use_graph(oww_ctx* h, int on);

#ifdef __cplusplus
}
#endif
#endif /* OWWHIP_H */
