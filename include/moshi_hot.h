// moshi_hot.h — C-ABI of the host-side driver of the streaming-decode hot path.
//
// In the reference this layer is libmoshi's C++ API (include/moshi/moshi.h:24-203): it builds the ggml
// graphs of the Temporal transformer, the chained Depth transformer and the Mimi codec once, then
// submits them every 80 ms frame. libmoshi itself stays the caller in a real
// deployment (it links this library's ggml surface unchanged); it cannot be built in
// this environment (SentencePiece / FFmpeg / model files are absent), so this driver restates the same
// graph construction and frame protocol — same op sequences, same upload / compute / read-back order —
// over synthetic weights, for the parity tests and for bench.py. Every function cites what it mirrors.
//
// Everything here runs on whichever ggml backend it is handed: the MI355X device, or the host device
// with the parity oracle attached (tests only).
#pragma once

#include "ggml.h"
#include "ggml-backend.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MOSHI_HOT_MAX_CODEBOOKS 33

// model hyper-parameters (tools/moshi-config.json keys; src/config.h:148-346)
struct moshi_hot_config {
    // Temporal transformer
    int32_t dim, num_heads, num_layers, ffn_hidden, context, max_period;
    int32_t text_card, card, n_q, dep_q;
    int32_t delays[MOSHI_HOT_MAX_CODEBOOKS];      // n_q + 1 entries
    // Depth transformer ("depformer")
    int32_t dep_dim, dep_heads, dep_layers, dep_ffn_hidden, dep_context;
    // weight storage types (ggml_type): linear layers / embedding tables
    int32_t linear_type, embed_type;
    // Mimi codec
    int32_t mimi_n_q;            // RVQ levels used by encoder and decoder (8 for moshi-sts)
    int32_t mimi_codebook_size;  // 2048
    int32_t enable_lm, enable_mimi_encoder, enable_mimi_decoder;
    // sampling: temp <= 0 -> greedy argmax (the parity mode, sampling.h:57-63)
    float   temp, temp_text;
    int32_t top_k, top_k_text;
    // model variants (all zero = moshika)
    int32_t personaplex;             // "model_type": "personaplex" (lm_default.h:223): the Depth graph chains dep_q (16) steps, the frame
                                     // protocol exposes 8 of them and takes the other speaker's 8 (lm.h:803-805); delay ring one row deeper (lm.h:728)
    int32_t extra_heads, extra_heads_dim;   // stt: linear heads on transformer_out; extra_heads[2] is the VAD head (lm.h:966-976)
    // tts (BASELINE.json configs[1])
    int32_t demux_second_stream;     // text embeddings E[id % (text_card+1)]·out1 + s·E[id / (text_card+1) - 1]·out2 (lm_utils.h:48-85)
    int32_t depformer_low_rank;      // width of the Depth embedding tables, followed by a low_rank linear to dep_dim (lm_utils.h:157-217); 0 = none
    int32_t delay_steps;             // Depth skipped while offset < delay_steps; tokens -1 until delays[q+1] + delay_steps (src/moshi.cpp:905, lm.h:915-921)
    int32_t cross_attention, cross_len;   // per-layer cross-attention over condition_cross F32[dim, cross_len] (transformer.h:343-396, 714-762)
    int32_t condition_sum;           // sum_condition F32[dim] added to the embedding sum (lm.h:579-581)
    int32_t dep_schedule_len;        // depformer_weights_per_step_schedule (lm_default.h:71-81); also the Depth ring capacity when dep_context == 0
    int32_t dep_schedule[MOSHI_HOT_MAX_CODEBOOKS];
    // synthetic weights only: standard deviation of the residual-update projections (out_proj, gating linear_out) relative to the
    // default 1/sqrt(fan_in); 0 = 1. Values < 1 give a CONTRACTIVE stack (every layer's update is small against the residual stream), on
    // which ggml's discontinuous roundings no longer compound chaotically: the parity tests then assert bit-exact greedy tokens and 1e-3
    // logits over many free-running frames at the full benchmark widths (same shapes, types and bytes moved).
    float   update_scale;
    // Depth-transformer codebook shard (lm.h:505-527, lm_default.h:136-146,187-216). dep_shard_world > 1: this model holds
    // the per-step Depth weight sets (depformer_in[k], in_projs[k], out_projs[k], gating[k], linears[k], depformer_emb[k-1]) of the steps
    // k with k % dep_shard_world == dep_shard_rank only - 1/world of the 375 MB - and runs the Depth chain as per-step graphs behind the
    // moshi_hot_depth_shard_* calls. depth_only: no Temporal stack, embeddings or codec at all (the ranks other than the Temporal owner).
    int32_t dep_shard_rank, dep_shard_world, depth_only;
    // Tensor-parallel Temporal stack (moshi_streaming_transformer_layer, transformer.h:910-1039). tp_world > 1: this model holds
    // rank tp_rank's SLICES of every Temporal layer - in_proj rows of its heads (q | k | v), the matching 1/N column block of out_proj, linear_in rows
    // [r F/N, (r+1) F/N) of both gate halves, the matching column block of linear_out - and its heads' KV rings; the stack runs as 2 L + 1 segment
    // graphs with a sum over ranks of one F32[dim] partial between them (moshi_hot_tp_* below). Column blocks fall on 256-value boundaries, so
    // the Q8_K activation blocks and every integer block dot are those of the unsplit layer; only the final float sums split.
    int32_t tp_rank, tp_world;
    // 1: the Mimi encode / decode graphs (and their scratch graphs) are built on a second command stream of the same GPU
    // (ggml_backend_mi355x_init_stream), so that moshi_hot_sts_pipeline_frame overlaps the codec of neighbouring frames with the LM step.
    // Ignored (one stream) on any other backend. Results are the same either way.
    int32_t codec_stream;
    // 1: the Depth graph takes the text token straight from the Temporal graph's sampler output in device memory and is queued right behind it - one host
    // wait per LM step instead of two - and the next frame's Temporal step inputs (mask row, RoPE phase, ring slot: functions of the stream position
    // only) are queued behind the Depth graph. Same graphs otherwise, same tokens. Not with a text hook, a Depth hook, demux or delay_steps (the
    // reference's host code inspects the text token between the two graphs there, lm.h:880-921).
    // 2: additionally the Temporal graph's embedding indices of the model's own codebooks are views of the same device-side token state, and
    // moshi_hot_sts_pipeline_frame runs AHEAD: step k is queued before step k - 1's tokens have been read (moshika-shaped models only; anything else
    // falls back to blocking steps behind the same calls).
    int32_t chain_depth;
    // moshi_hot_create_streams / moshi_hot_create_slots: 0 = at most MOSHI_HOT_DEFAULT_MAX_STREAMS (16) columns, the limit every configuration written
    // before wide batches existed keeps; 1 = up to MOSHI_HOT_MAX_STREAMS (64). A caller opts in because a column is not free: its K / V rings are
    // 2 x num_layers x dim x context BF16 values of device memory (1.57 GB at moshika's widths and context 3000). Nothing else depends on it.
    int32_t wide_streams;
    // moshi_hot_create_streams / moshi_hot_create_slots with personaplex = 1: 0 = NULL for B > 1, as before PersonaPlex columns existed; 1 = the PersonaPlex
    // shape of a B > 1 model ("PersonaPlex streams and slots" below). 1 without personaplex = 1, or beside anything the moshika shape excludes: NULL.
    // Ignored by a single-stream model. (It sits in front of float_accumulate, which tests/test_float_acc_streams_gpu.py pins as the struct's last field.)
    int32_t persona_columns;
    // 1: moshi_hot_create / _create_streams / _create_slots / _create_from_gguf switch the handle the model is created on (and its codec sibling stream,
    // if one is made) to the float-accumulating mat-mul, ggml_backend_mi355x_set_float_accumulate(backend, 1): every B-column product of BF16 / F16
    // linears - streams and slots steps, moshi_hot_slots_prefill / _long, moshi_hot_slots_replay, the [dim, T] passes of moshi_hot_prefill - sums in
    // float on the BF16 / F16 matrix unit instead of in double. Single-column products, F32 weights, the ring products and the codec stay where they
    // are. Ignored on any other backend. The setting belongs to the HANDLE, as wide_streams' sampler width does: a model never lowers it, models
    // created on the handle later run in this mode too, and a caller who wants both contracts in one process uses two handles.
    // Contract with 1: a BF16 / F16 model is no longer bit-comparable with the CPU reference (sums of K exact products in float, not in double). It
    // stays bit-reproducible (same inputs, same bits) and column-independent (the same conversation in any column of any B, prefilled in any chunk,
    // gets the same bits); snapshots, prefill and replay continue bit for bit on the same backend and mode.
    int32_t float_accumulate;
};

typedef struct moshi_hot_model moshi_hot_model_t;

// fills cfg with tools/moshi-config.json (moshika-7B) under `-q q4_k`: Q4_K linears, Q4_0 embeddings
GGML_API void moshi_hot_config_moshika(struct moshi_hot_config * cfg);
// tools/personaplex-config.json under `-q q4_k` (BASELINE.json configs[4]; run with context 2000 there)
GGML_API void moshi_hot_config_personaplex(struct moshi_hot_config * cfg);

// allocates weights (synthetic, deterministic in `seed`), persistent state (KV rings, conv tails) and
// the scratch contexts on `backend` (moshi_alloc / mimi_alloc / moshi_lm_load / moshi_lm_start,
// src/moshi.cpp:88-130, 851-898)
GGML_API moshi_hot_model_t * moshi_hot_create(ggml_backend_t backend, const struct moshi_hot_config * cfg, uint64_t seed);
GGML_API void moshi_hot_free(moshi_hot_model_t * m);

// ---- lockstep streams: B conversations stepped together over one set of weights ------------------------------------------------------------
// The reference's batch dimension (moshi_kv_cache_state's batch_size, transformer.h:155-171, fixed to 1 at :326-328) made real: activations are
// [dim, 1, B], the KV rings [D, capacity, H, B], the token inputs B per codebook. Each column holds one conversation with its own delay ring
// (lm.h:715-743), its own KV ring rows, its frame count and its stream position. Every weight is read once per step for all B columns. A lockstep
// model and a slots model (below) are this one model and step alike; they differ only in where a column's position comes from. Here every column
// is open from creation and all B share one stream position, so the mask row, the RoPE phase and the ring slot are common.
// n_streams == 1 builds exactly moshi_hot_create's model.
// n_streams > 1 takes the LM alone: enable_lm = 1 with both codec halves off, personaplex = 0 (or persona_columns = 1 beside it), tp_world == 0, dep_shard_world <= 1, depth_only == 0,
// chain_depth == 0, codec_stream == 0, and 1 <= n_streams <= 16 (wide_streams = 1: <= MOSHI_HOT_MAX_STREAMS), in one of three shapes (demux / cross-attention / condition_sum / low-rank embeddings /
// weight schedule / delay_steps: on the tts shape only, see "tts streams and slots" below):
//  * the moshika shape: dep_q > 0, n_q > dep_q, extra_heads == 0;
//  * the stt shape (moshi-stt): dep_q == 0 and n_q > 0 - no Depth transformer, every audio codebook is an input, the text token comes from the
//    Temporal head - with extra_heads == 0, or extra_heads >= 1 heads of 1 <= extra_heads_dim <= 16 values on transformer_out (lm.h:966-976).
//    A frame takes n_q codes per column, out_audio is not touched and may be NULL, the frame's only sampler site is 0 (the text head), and the
//    heads' probabilities of every column are computed by the Temporal graph itself and read back with the tokens (moshi_hot_last_heads).
//  * the tts shape (moshi-tts): dep_q > 0, n_q == dep_q, extra_heads == 0.
//  * the PersonaPlex shape (personaplex = 1 AND persona_columns = 1; personaplex = 1 alone keeps returning NULL): dep_q >= 8, n_q >= dep_q, n_q > 8,
//    extra_heads == 0 - see "PersonaPlex streams and slots" below.
// Anything else returns NULL, and so does a B > 1 model whose state (chiefly the K / V rings: 2 x layers x dim x context BF16 values per column, 1.57 GB
// at moshika's widths and context 3000) cannot be allocated on the device: nothing is left behind, the caller may ask for fewer columns.
// On such a model moshi_hot_read_last("text_logits" | "transformer_out" | "dep_logits<k>") returns B consecutive rows (stream 0 first), and
// moshi_hot_set_context_fill moves the shared stream position, not the delay rings. The single-stream frame calls (moshi_hot_lm_step*, moshi_hot_sts_*,
// moshi_hot_ring_bytes, moshi_hot_host_ring, moshi_hot_layer_probe) return -1, and the calls without a result (moshi_hot_mimi_*, moshi_hot_prefill,
// moshi_hot_personaplex_system_prompts*, moshi_hot_lm_step_embedding, moshi_hot_fill_ring, moshi_hot_force_last, moshi_hot_set_conditions, the hooks,
// moshi_hot_depth_shard_* and moshi_hot_tp_*) do nothing; moshi_hot_depth_shard_msg / _tout and moshi_hot_tp_msg return NULL.
#define MOSHI_HOT_MAX_STREAMS 64           // columns of one streams or slots model with wide_streams = 1: what one pass of the batched mat-muls takes
#define MOSHI_HOT_DEFAULT_MAX_STREAMS 16   // ... and with wide_streams = 0
GGML_API moshi_hot_model_t * moshi_hot_create_streams(ggml_backend_t backend, const struct moshi_hot_config * cfg, uint64_t seed, int n_streams);
// one frame of every stream (moshi_lmgen_step, lm.h:778-979, B times in lockstep): in_audio = B x (n_q - dep_q) codes (stream-major), text_token = B,
// out_audio = B x dep_q (stream-major). Returns 1 when every stream's outputs are valid, else 0: while the delay rings fill (the same for every
// stream; nothing is written) or when an audio token is -1 (every stream's outputs are written). -1 on a slots model; moshi_hot_lm_step when B = 1.
GGML_API int moshi_hot_lm_step_streams(moshi_hot_model_t * m, const int32_t * in_audio, int32_t * text_token, int32_t * out_audio);
GGML_API int moshi_hot_n_streams(moshi_hot_model_t * m);

// ---- stream slots: B independent conversations over one set of weights, admitted and retired mid-batch ----------------------------------------
// The B-column model of moshi_hot_create_streams with a stream position per column: slot b's mask row, RoPE phase and ring slot follow its own
// position, so a conversation can start in any frame while the others run on. Same configurations as moshi_hot_create_streams, 2 <= n_slots <= 16 (wide_streams = 1: <= MOSHI_HOT_MAX_STREAMS);
// anything else returns NULL (one conversation: moshi_hot_create). All slots start closed.
// A closed slot still occupies its column: it is stepped frozen at its position, fed the initial tokens, writes only its own KV ring rows, and its
// results are discarded. moshi_hot_read_last returns B rows and moshi_hot_n_streams returns B, as on a streams model. The single-stream calls and
// moshi_hot_lm_step_streams refuse as on a streams model (moshi_hot_lm_step_streams returns -1); moshi_hot_set_context_fill does nothing.
GGML_API moshi_hot_model_t * moshi_hot_create_slots(ggml_backend_t backend, const struct moshi_hot_config * cfg, uint64_t seed, int n_slots);
// slot b starts a new conversation at stream position 0 with the delay ring of a fresh stream. Its KV ring rows are NOT cleared: the mask row of
// position p admits ring slots 0..p only, each rewritten by the new conversation before it is admitted, so the previous occupant's rows are never
// read. Returns 0, or -1 for a bad index or a model that is not a slots model.
GGML_API int moshi_hot_slot_open(moshi_hot_model_t * m, int b);
GGML_API int moshi_hot_slot_close(moshi_hot_model_t * m, int b);   // 0, or -1 as moshi_hot_slot_open
// slot b's stream position: frames stepped since it was opened (unless moshi_hot_slot_set_fill moved it), -1 if it is closed or b is bad
GGML_API int64_t moshi_hot_slot_position(moshi_hot_model_t * m, int b);
// moshi_hot_set_context_fill for one slot (long-context tests and benchmarks): moves slot b's stream position only, not its delay ring
GGML_API void moshi_hot_slot_set_fill(moshi_hot_model_t * m, int b, int64_t offset);
// one frame of every slot. Layouts as moshi_hot_lm_step_streams; the codes of closed slots are ignored. status = B entries: 1 when slot b's outputs
// are valid, 0 while its own delay ring fills, -1 when it is closed; the outputs of a slot whose status is not 1 are written as -1. Returns the
// number of slots with status 1, or -1 on a model that is not a slots model. With no slot open it does no device work and returns 0.
GGML_API int moshi_hot_lm_step_slots(moshi_hot_model_t * m, const int32_t * in_audio, int32_t * text_token, int32_t * out_audio, int32_t * status);
// The extra heads of the last step of a B > 1 stt-shaped model (lockstep or slots): out[(b * extra_heads + k) * extra_heads_dim + i] = probability i of
// soft_max(extra_heads[k] . transformer_out) of column b - B x extra_heads x extra_heads_dim floats, column-major by column. The VAD value the reference
// reports (lm.h:966-976) is out[(b * extra_heads + 2) * extra_heads_dim]. The rows of a column whose status in that step was not 1 (closed, held, its
// delay ring still filling) are -1. Returns the number of floats written, or -1 (nothing written) on a single-stream model, on a model without extra
// heads, or when n is smaller than that count.
GGML_API int moshi_hot_last_heads(moshi_hot_model_t * m, float * out, int64_t n);
// Slot prefill: admit conversations that already have a history. Job j advances open slot slots[j] by n_frames[j] provided frames (tokens[j]:
// n_frames[j] x (n_q + 1), text first - what moshi_hot_prefill takes), leaving the slot as a fresh single-stream model is after moshi_hot_prefill over
// the same frames: delay ring, frame count (the frame the seeded noise source sees), stream position, the slot's KV ring rows and its row of
// transformer_out. The rows of all jobs are laid end to end in job order and cut into [dim, T] passes of at most `chunk` rows (< 1 or > 64: 64): a
// job may span passes, a pass may hold several jobs - the weights stream once per pass whatever the number of jobs. Nothing outside the jobs' own
// columns is touched. Returns the number of frames prefilled (0 with no device work for n_jobs == 0 or no frames at all), or -1 with no state changed
// when the model is not a slots model, n_jobs > B, a slot index is bad, closed or named twice, or a job would pass the ring's end
// (position + n_frames > context: the T > 1 mask is causal only before the wrap; moshi_hot_slots_prefill_long below takes such a job).
GGML_API int moshi_hot_slots_prefill(moshi_hot_model_t * m, int n_jobs, const int32_t * slots, const int32_t * const * tokens, const int32_t * n_frames, int chunk);
GGML_API int moshi_hot_slot_prefill(moshi_hot_model_t * m, int b, const int32_t * tokens, int n_frames, int chunk);   // one job
// Slot prefill past the ring's end: arguments, return values and refusals of moshi_hot_slots_prefill / _slot_prefill, except that position + n_frames has
// no upper bound - a job may cross the ring's end, start at or past `context` (a slot stepped live past the wrap) and go round the ring several times.
// The contract is the same: afterwards the slot is what a fresh single-stream model is after moshi_hot_prefill over the same frames, which steps single
// provided frames at and after the wrap - bit for bit on the oracle for every `chunk`. A job's rows before the ring's end run as above (a piece that would
// cross it stops there and closes its pass); its rows at and past it are RING-ORDERED: inside every layer they run one by one in row order, each writing
// ring row position % context and attending under the mask row of a live step at its position, while the projections, norms and the FFN stay one call
// over all rows of the pass. A pass holds at most 16 ring-ordered rows. With no job past the ring's end the passes, graphs and plans are those of
// moshi_hot_slots_prefill. moshi_hot_slot_hold works between calls as above (past the wrap the frozen step's write lands on the row of position - context,
// which leaves the window in the frame that writes `position`).
GGML_API int moshi_hot_slots_prefill_long(moshi_hot_model_t * m, int n_jobs, const int32_t * slots, const int32_t * const * tokens, const int32_t * n_frames, int chunk);
GGML_API int moshi_hot_slot_prefill_long(moshi_hot_model_t * m, int b, const int32_t * tokens, int n_frames, int chunk);   // one job
// hold != 0: moshi_hot_lm_step_slots steps open slot b as it steps a closed one (fed the initial tokens at its frozen position, nothing of its column
// advances; only ring row position % context of its own column is written, which the next prefill row or live frame rewrites before a mask row admits
// it) and reports status -2 with outputs -1 - a long history can be prefilled one pass at a time between the frames of the live slots. hold == 0
// releases it; moshi_hot_slot_open / _close clear the hold. Returns 0, or -1 for a bad index, a closed slot or a model that is not a slots model.
GGML_API int moshi_hot_slot_hold(moshi_hot_model_t * m, int b, int hold);
// Slot snapshots: fork, save and restore a conversation without recomputing it. A conversation's state is its column record (delay ring, frame count,
// stream position), its sampling setting with the seeded flag, its row of transformer_out and the LIVE rows of its column of every Temporal K and V ring:
// ring rows 0 .. n - 1 of every head with n = min(position, context) - before the wrap the mask admits no other row, after it all of them. The Depth rings
// start afresh every frame (the chained Depth graph rewrites every row it reads) and carry nothing between frames: they are not part of a snapshot.
// A snapshot works at any position, past the ring's end included (where moshi_hot_slots_prefill refuses and moshi_hot_slots_prefill_long recomputes), costs one copy of those rows instead of a
// recomputation, and the restored or forked slot continues bit for bit - sampled conversations included, which prefill cannot reproduce. The calls block;
// no other slot's rings, delay ring, position, hold or sampling state is touched. Each returns -1 and changes nothing on a model that is not a slots
// model, for a bad index, and where a slot is not in the state the call requires.
//  * fork: src open (a held slot counts as open), dst closed and != src. Afterwards dst is open, not held, and holds a copy of src's state: fed the same
//    codes both slots produce the same conversation. A caller that wants sampled branches to diverge sets a new seed on dst (moshi_hot_set_sampling).
//  * save: slot b open. Writes a self-describing blob - a magic, a format version, a fingerprint of the configuration (dim, heads, layers, context, n_q,
//    dep_q, card, text_card, the delays, the ring type BF16, sampled or greedy), the host state, transformer_out, then per layer K and then V as
//    H x n x D BF16 - and returns the bytes written; buf == NULL: the bytes needed now (they grow with the position until the ring is full). -1 when
//    nbytes is too small. The slot is unchanged.
//  * load: slot b closed; nbytes must be the blob's exact size (a truncated or oversized buffer is refused, as are a wrong magic, version or
//    fingerprint). The blob may come from any column of a slots model of any B on any backend with the same fingerprint. Afterwards the slot is open,
//    not held, and holds that conversation, its sampling setting included.
GGML_API int     moshi_hot_slot_fork(moshi_hot_model_t * m, int src, int dst);
GGML_API int64_t moshi_hot_slot_save(moshi_hot_model_t * m, int b, void * buf, int64_t nbytes);
GGML_API int     moshi_hot_slot_load(moshi_hot_model_t * m, int b, const void * buf, int64_t nbytes);

// ---- tts streams and slots: B text-to-speech conversations ------------------------------------------------------------------------------------
// The tts shape of a B > 1 model: dep_q > 0 and n_q == dep_q - no codebook is an input (in_audio may be NULL), every column brings a voice
// (condition_cross, condition_sum) and a text stream. On this shape alone, in any combination: cross_attention (cross_len >= 1), condition_sum,
// demux_second_stream, depformer_low_rank, dep_schedule_len > 0 (dep_context == 0: ring = schedule length) and delay_steps >= 0, applied per column by the
// column's own frame count: while it is below delay_steps the column is REPLACED (src/moshi.cpp:905, lm.h:910-921: its Depth tokens are -1, nothing is read
// out; the Depth graph is skipped when every stepping column is replaced), and audio[q] = -1 while it is below delays[q + 1] + delay_steps.
// moshi_hot_slots_prefill / _slot_prefill (and their _long forms) and moshi_hot_slot_fork / _save / _load return -1 on this shape and change nothing: a
// history goes in through moshi_hot_slots_replay, a snapshot is taken with moshi_hot_slot_fork_full / _save_full / _load_full (below).
//
// Column b's conditions (the B > 1 form of moshi_hot_set_conditions, which does nothing on such a model): sum F32[dim] and cross F32[dim * cross_len], either
// may be NULL to leave that half as it is. cross also runs init() (transformer.h:343-396) for column b of every layer's K / V. The setting belongs to
// the column as the sampling setting does: it may be set on an open or a closed slot, holds from the next step on and survives moshi_hot_slot_close /
// _open; no other column's state is touched. A column never set has zero conditions (a single-stream model before moshi_hot_set_conditions).
// Returns 0, or -1 on a single-stream model, for a bad column, or when the model has no condition of the kind given.
GGML_API int moshi_hot_set_conditions_column(moshi_hot_model_t * m, int b, const float * sum, const float * cross);
// moshi_hot_lm_step_streams / _slots with the text stream from above the boundary (the B-column form of moshi_hot_set_text_hook: the TTS state machine
// hands this frame's token of every column in): text_in = B values or NULL. text_in[b] != MOSHI_HOT_TEXT_KEEP replaces column b's sampled text token where
// on_text_hook does (lm.h:880-900): after the Temporal graph, before the Depth graph and the delay ring's write. Values of closed or held columns are
// ignored; text_in == NULL is the plain call. They work on every B > 1 shape (moshika shape: a forced text token); in_audio may be NULL on the tts shape.
// Returns as the plain calls; moshi_hot_lm_step_streams_text returns -1 on a single-stream model too.
#define MOSHI_HOT_TEXT_KEEP INT32_MIN
GGML_API int moshi_hot_lm_step_streams_text(moshi_hot_model_t * m, const int32_t * in_audio, const int32_t * text_in, int32_t * text_token, int32_t * out_audio);
GGML_API int moshi_hot_lm_step_slots_text(moshi_hot_model_t * m, const int32_t * in_audio, const int32_t * text_in, int32_t * text_token, int32_t * out_audio, int32_t * status);

// Replay: a tts-shaped slots model has no provided frames (n_q == dep_q: needed_tokens == 0, lm.h:807-809), so a history is the frames a conversation
// COMMITTED: n_q + 1 tokens each, the text value (what text_in gave, a demuxed pair as one value) and then the dep_q raw audio samples of the frame, the
// -1 of delay_steps (lm.h:910-921) included - what moshi_hot_slot_last_raw returns after a live frame. The tokens are taken verbatim, as the
// reference's text_prefixes / audio_prefixes override a frame's samples (lm.h:883-885, 922-930): a forced voice prefix and a recorded conversation are
// the same call. Arguments, return values, passes and refusals of moshi_hot_slots_prefill_long, on a tts-shaped slots model only (any other model: -1,
// nothing changes). Per frame the column's model inputs are read from its delay ring as a live step reads them (lm.h:826-834), the frame's tokens are
// written to it (lm.h:935-943), the frame count and the stream position advance; no Depth graph runs and no sampler noise is drawn. Afterwards the slot is
// what a fresh single-stream model with the same conditions is after n_frames steps with moshi_hot_force_last(text_f, audio_f) after each: delay ring,
// frame count, stream position, its column's rows of every Temporal K / V ring and its row of transformer_out - on the oracle the frames that follow are
// that model's bit for bit, for every chunk and any number of jobs per pass. The rows of a pass run moshi_streaming_transformer_layer
// (transformer.h:910-1039) with the cross-attention (transformer.h:714-762, 936-944) of every job against its own column's condition, the condition sum
// (lm.h:579-581) of its column and the demuxed text embedding (lm_utils.h:48-66).
GGML_API int moshi_hot_slots_replay(moshi_hot_model_t * m, int n_jobs, const int32_t * slots, const int32_t * const * tokens, const int32_t * n_frames, int chunk);
GGML_API int moshi_hot_slot_replay(moshi_hot_model_t * m, int b, const int32_t * tokens, int n_frames, int chunk);   // one job
// The n_q + 1 tokens slot b committed in its latest frame (row `frames` of its delay ring, lm.h:935-943): the text, then the raw audio tokens. The delayed
// read-out of a step lags by max(delays) frames (lm.h:950-964), so this is what a server logs per frame to hold the history that replay takes. Any slots
// model. Returns 0, or -1 for a bad or closed slot, a slot that has stepped no frame yet, or a model that is not a slots model.
GGML_API int moshi_hot_slot_last_raw(moshi_hot_model_t * m, int b, int32_t * tokens);
// Snapshots that carry the conditions: signatures, states and refusals of moshi_hot_slot_fork / _save / _load. On a model that is not tts-shaped they ARE
// those calls (same graphs, same bytes). On the tts shape a conversation's state also holds its column of cond_sum and cond_cross and of every layer's
// cross-attention K / V (transformer.h:343-396); the destination column's own conditions are overwritten. fork copies all of it on the device. save writes
// blob version 2 - the fingerprint also mixes cross_attention, cross_len, condition_sum, demux_second_stream and delay_steps; cond_sum (dim F32) and
// cond_cross (dim x cross_len F32) follow transformer_out where the model has them - and load uploads both and runs init() for the column as
// moshi_hot_set_conditions_column does: on the backend that saved it the copy continues bit for bit, on another as a conversation with those conditions
// does there. A version-1 blob, a blob of another shape or cross_len, a truncated or an oversized one is refused and changes nothing.
GGML_API int     moshi_hot_slot_fork_full(moshi_hot_model_t * m, int src, int dst);
GGML_API int64_t moshi_hot_slot_save_full(moshi_hot_model_t * m, int b, void * buf, int64_t nbytes);
GGML_API int     moshi_hot_slot_load_full(moshi_hot_model_t * m, int b, const void * buf, int64_t nbytes);

// ---- PersonaPlex streams and slots: B PersonaPlex conversations, personas admitted in batched passes -----------------------------------------------
// The PersonaPlex shape of a B > 1 model (personaplex = 1 and persona_columns = 1, the LM alone, no tts flag, no extra heads, no tensor parallelism, Depth
// shard, chain_depth or codec_stream). The Depth graph chains all dep_q (16) steps per column; the frame protocol is the single-stream one per column
// (lm.h:802-805): moshi_hot_lm_step_streams / _slots take B x 8 codes of the other speakers (in_audio, stream-major) and write B x 8 codes (out_audio),
// the delay ring is one row deeper (lm.h:728) and takes all 16 raw samples. moshi_hot_slot_last_raw returns n_q + 1 tokens as on every slots model.
// moshi_hot_slots_prefill / _long, moshi_hot_slot_hold and moshi_hot_slot_fork / _save / _load work as on the moshika shape (the blob's fingerprint
// mixes the flag in: a moshika-shaped blob is refused here and the other way round); moshi_hot_slots_replay is the tts shape's and refuses; the _full snapshot calls are the plain calls here, as on every shape but the tts one.
//
// A conversation starts with a PERSONA (moshi_lmgen_step_system_prompts, lm.h:1120-1134): n_voice voice-prompt frames whose Temporal input is a
// precomputed embedding (lm.h:1004-1036), the voice's image of the delay ring (lm.h:1038-1052), `silence` silence frames, the text prompt, `silence`
// silence frames - a few hundred frames. moshi_hot_slots_persona runs them as batched [dim, T] passes:
struct moshi_hot_persona {
    const void * voice; int32_t voice_type; int32_t n_voice;   // n_voice rows of [dim] values, GGML_TYPE_F32 / BF16 / F16 (lm.h:1016 casts to F32); NULL / 0: none
    const int32_t * prompt_cache;                               // moshi_hot_host_ring's layout, rows x (n_q + 1); NULL: the ring stays as it is (lm.h:1038-1052)
    const int32_t * text_prompt; int32_t n_text;                // lm.h:1079-1098
    int32_t silence;                                            // frames of moshi_lmgen_step_audio_silence before and after the text prompt (the tool: 6); 0: none
};
// Job j advances open slot slots[j] by n_voice + silence + n_text + silence rows, in that order. A voice row's Temporal input is row t of the voice,
// exactly converted to F32; on the host it advances the frame count and the stream position only (nothing enters the delay ring). After the last voice
// row prompt_cache, if given, replaces the delay ring's rows (the frame count stays; a persona without voice rows takes it ahead of its first row, and one
// with no rows at all still takes it: the call then changes that slot's delay ring and counts 0 rows for it). The other rows are the provided frames that
// moshi_hot_personaplex_system_prompts steps: PROMPT_TOKENS, the text replaced on the text-prompt rows. No Depth graph runs and no sampler noise is
// drawn (the single-stream calls compute and discard both). The rows of all jobs go end to end into passes of at most `chunk` rows (< 1 or > 64: 64),
// cut as moshi_hot_slots_prefill cuts them; a job's piece of a pass is one attention sequence whatever its rows are. Afterwards the slot is what a
// fresh single-stream PersonaPlex model is after n_voice x moshi_hot_lm_step_embedding, moshi_hot_set_host_ring(prompt_cache) and
// moshi_hot_personaplex_system_prompts (with `silence` = 6): delay ring, frame count, stream position, its column's rows of every Temporal K / V ring
// and its row of transformer_out - on the oracle, greedy, the frames that follow are that model's bit for bit, for every chunk and any number of jobs
// per pass. moshi_hot_slot_hold works between calls as for prefill. Returns the number of rows, or -1 with nothing changed: a model that is not a
// PersonaPlex-shaped slots model, n_jobs > B, a bad, closed or repeated slot, a bad persona (a negative count, a count without its pointer, a voice
// type other than the three), or position + rows > context (a persona that passes the ring's end is not supported).
GGML_API int moshi_hot_slots_persona(moshi_hot_model_t * m, int n_jobs, const int32_t * slots, const struct moshi_hot_persona * personas, int chunk);
GGML_API int moshi_hot_slot_persona(moshi_hot_model_t * m, int b, const struct moshi_hot_persona * persona, int chunk);   // one job
// Persona caching: a persona costs a few passes once - admit it into a spare slot, moshi_hot_slot_save the slot, and moshi_hot_slot_load the blob into a
// closed slot for every caller that wants that persona (one copy of the ring rows instead of the passes).

// ---- decoder slots: the Mimi decode of B conversations in one pass ---------------------------------------------------------------------------------
// The codec's counterpart of a slots model: one set of decoder weights, B columns, each a conversation's streaming decoder state - conv tails and
// transposed-conv partials [len, C, B], the decoder transformer's K / V rings [D, 250, H, B] and a position of its own. The graph is mimi_decode's
// (compression.h:156-187) with the reference's batch dimension made real; the four SEANet transposed convolutions, which ggml takes as matrices only,
// are B matrix nodes on the column views. On the oracle slot b's PCM is bit-identical to a fresh single-stream codec-only model (moshi_hot_create with
// enable_lm = 0) fed the same codes frame by frame, whatever the other slots do.
// Requires enable_lm = 0, enable_mimi_decoder = 1, enable_mimi_encoder = 0, codec_stream = 0 and 2 <= n_slots <= 16 (wide_streams = 1:
// <= MOSHI_HOT_MAX_STREAMS); anything else, or a state that does not fit the device, returns NULL. The weights are those moshi_hot_create makes for
// the same cfg and seed, under the same names. All slots start closed. moshi_hot_n_streams returns B. Every other frame call (moshi_hot_mimi_decode /
// _encode, moshi_hot_lm_step*, moshi_hot_sts_*, the LM slot calls) refuses as on a B > 1 LM model; the calls below return -1 (or do nothing) on any other model.
GGML_API moshi_hot_model_t * moshi_hot_create_codec_slots(ggml_backend_t backend, const struct moshi_hot_config * cfg, uint64_t seed, int n_slots);
// slot b starts a new conversation: column b of every conv tail and transposed-conv partial is zeroed, its decoder-transformer position is 0. Its
// ring rows are not cleared (the mask admits only rows the new conversation has written). Returns 0, or -1 for a bad index or another kind of model.
GGML_API int moshi_hot_codec_slot_open(moshi_hot_model_t * m, int b);
GGML_API int moshi_hot_codec_slot_close(moshi_hot_model_t * m, int b);   // 0, or -1 as moshi_hot_codec_slot_open
// frames decoded since slot b was opened (unless moshi_hot_codec_slot_set_fill moved it), -1 if it is closed or b is bad
GGML_API int64_t moshi_hot_codec_slot_position(moshi_hot_model_t * m, int b);
// moves slot b's decoder-transformer position only, in frames (2 ring rows each), not its conv states (tests and benchmarks)
GGML_API void moshi_hot_codec_slot_set_fill(moshi_hot_model_t * m, int b, int64_t frames);
// one frame of every open slot: codes = B x mimi_n_q (slot-major), pcm = B x 1920, status = B entries: 1 for a decoded slot, -1 for a closed one, whose
// codes are ignored and whose pcm row is written as zeros (it is computed frozen on code 0; the next open resets its state). Returns the number of
// slots decoded; 0 with no device work when none is open; -1 with nothing changed on another kind of model or when an open slot has a code outside
// [0, mimi_codebook_size).
GGML_API int moshi_hot_mimi_decode_slots(moshi_hot_model_t * m, const int32_t * codes, float * pcm, int32_t * status);

// ---- encoder slots: the Mimi encode of B conversations in one pass ---------------------------------------------------------------------------------
// The other half of the codec at B columns: one set of encoder weights, B columns, each a conversation's streaming encoder state - the conv tails
// [len, C, B] of the SEANet encoder and of the downsampler, the encoder transformer's K / V rings [D, 250, H, B] and a position of its own. The graph
// is mimi_encode's (compression.h:284-308) with the batch dimension made real: the frame is [1920, 1, B], the transformer takes 2 rows per column,
// and every residual-VQ level searches its codebook for the B residuals at once (distances [NC, B], one code per column). On the oracle slot b's codes
// and both projected latents are bit-identical to a fresh single-stream codec-only model (moshi_hot_create with enable_lm = 0) fed the same frames one
// by one, whatever the other slots do.
// Requires enable_lm = 0, enable_mimi_encoder = 1, enable_mimi_decoder = 0, codec_stream = 0, mimi_n_q >= 1, mimi_codebook_size >= 1 and
// 2 <= n_slots <= 16 (wide_streams = 1: <= MOSHI_HOT_MAX_STREAMS); anything else, or a state that does not fit the device, returns NULL. The weights
// are those moshi_hot_create makes for the same cfg and seed, under the same names. All slots start closed. moshi_hot_n_streams returns B.
// moshi_hot_codec_slot_open / _close / _position / _set_fill take such a model as they take a decoder-slots model: open zeroes column b of every
// encoder conv tail and sets its encoder-transformer position to 0 (ring rows stay: the mask admits written rows only), set_fill moves the position
// alone. Every other frame call refuses: moshi_hot_mimi_encode / _decode do nothing, moshi_hot_mimi_decode_slots, moshi_hot_lm_step*, moshi_hot_sts_*
// and the LM slot calls return -1. moshi_hot_read_last("enc_latent_first" | "enc_latent_rest") returns B consecutive rows of 256, slot 0 first.
GGML_API moshi_hot_model_t * moshi_hot_create_encoder_slots(ggml_backend_t backend, const struct moshi_hot_config * cfg, uint64_t seed, int n_slots);
// one frame of every open slot: pcm = B x 1920 (slot-major), codes = B x mimi_n_q, status = B entries: 1 for an encoded slot, -1 for a closed one, whose
// pcm is ignored and whose codes row is written as -1 (it is computed frozen on zero PCM at its position, which does not advance; the next open resets
// its state). Returns the number of slots encoded; 0 with no device work when none is open (codes are then all -1); -1 on any other kind of model,
// decoder-slots models included, or on a NULL argument.
GGML_API int moshi_hot_mimi_encode_slots(moshi_hot_model_t * m, const float * pcm, int32_t * codes, int32_t * status);

// ---- codec slot snapshots: fork, save and restore a decoder or an encoder slot -----------------------------------------------------------------------
// The codec's counterpart of moshi_hot_slot_fork / _save / _load, on a decoder-slots or an encoder-slots model: same signatures, same blocking behaviour,
// same refusal style. A streaming codec state depends on its whole history and the codec has no prefill call, so a copy is the only way to move or
// branch it. The state of column b: its position (frames); column b of every carried conv state, the tensors moshi_hot_codec_slot_open clears, in model
// order (a decoder: upsample.prev, the two conv tails, the four transposed-conv partials, block1.prev of the four residual blocks; an encoder: the six
// conv tails, block1.prev of the four residual blocks, downsample.prev - eleven each); and ring rows 0 .. n - 1 of every head of column b of every K
// and V ring of the codec transformer, n = min(position x rows per frame, capacity) = min(2 position, 250). Before the wrap the mask admits only
// written rows, after it all 250 are live; a column positioned by moshi_hot_codec_slot_set_fill has live rows nobody wrote, copied like any other.
// No other column's state is touched. Each call returns -1 and changes nothing on any other kind of model (as moshi_hot_slot_fork / _save / _load
// keep doing on these), for a bad index, and where a slot is not in the state the call requires.
//  * fork: src open, dst closed and != src. Afterwards dst is open at src's position and, given the same input, yields the same output from then on.
//  * save: slot b open. Writes a self-describing little-endian blob and returns the bytes written; buf == NULL: the bytes needed now (they grow by
//    2 x layers x dim x 2 x rows per frame per frame until the ring is full); -1 when nbytes is too small. The slot is unchanged. The blob: magic "MCSL",
//    format version 1, kind (1 decoder, 2 encoder), a reserved zero, a fingerprint (FNV-1a over the kind, the codec transformer's dim, heads, layers,
//    capacity, rows per frame and ring type, and the (len, C) of every carried state in model order), total bytes, position, n - 48 bytes - then every
//    state's column as F32 [len, C], each zero-padded to a multiple of 16 bytes, then per layer K and then V as H x n x D BF16. The same state always
//    gives the same bytes.
//  * load: slot b closed; nbytes must be the blob's exact size. A NULL or short header, a truncated or oversized buffer, a wrong magic, version, kind
//    or fingerprint, a non-zero reserved field, a negative position and an n that does not follow from the position are refused before anything
//    changes. The blob may come from any column of a model of the same kind of any B on any backend with the same fingerprint. Afterwards the slot is
//    open at the blob's position and holds that conversation.
GGML_API int     moshi_hot_codec_slot_fork(moshi_hot_model_t * m, int src, int dst);
GGML_API int64_t moshi_hot_codec_slot_save(moshi_hot_model_t * m, int b, void * buf, int64_t nbytes);
GGML_API int     moshi_hot_codec_slot_load(moshi_hot_model_t * m, int b, const void * buf, int64_t nbytes);

// ---- per-conversation sampling: a seed, temperatures and top-k values per column --------------------------------------------------------------------
// In sampled mode (config temp > 0 and temp_text > 0) the sampler divides the top-k probabilities by Exp(1) noise that the host uploads per compute
// (src/context.h:456-480, moshi/utils/sampling.h:4-64). By default that noise comes from libc rand() in one sweep over the whole [k, B] tensor, so a
// conversation's draws depend on B, on its column and on the frame it was admitted in. A SEEDED column draws from a counter-based source instead:
//
//   noise(seed, frame, site, rank) = -logf(u) / lambd                                  (lambd = 1 at every sampler site)
//   u = (float) (2 * (z >> 41) + 1) * 2^-24                                             (an odd multiple of 2^-24: 0 < u < 1, the noise is finite and > 0)
//   z = mix(mix(seed + 0x9E3779B97F4A7C15) ^ (frame * 0xD1342543DE82EF95 + (site << 32 | rank)))                       (64-bit wrap-around arithmetic)
//   mix(x): x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9;  x = (x ^ (x >> 27)) * 0x94D049BB133111EB;  return x ^ (x >> 31)   (SplitMix64's output function)
//
// frame = the conversation's own frame count (frames stepped since the slot was opened; frames stepped by a lockstep or single-stream model), site = 0
// for the text head and 1 + k for Depth step k, rank = the index into the top-k row. Nothing else enters: a conversation with a given seed gets the same
// tokens in any column of any B beside any neighbours, and the tokens of a fresh single-stream model configured and seeded alike.
struct moshi_hot_sampling { uint64_t seed; float temp, temp_text; int32_t top_k, top_k_text; };
// Sets column b's sampling from its next frame on. Returns 0, or -1 (nothing changes) on a greedy model, for a bad column or for values out of range.
//  * B > 1 (slots and lockstep models): temp > 0, temp_text > 0, 1 <= top_k <= config.top_k, 1 <= top_k_text <= config.top_k_text - the configuration's
//    top-k values are the compiled maximum (the graph keeps that many rows; a column with fewer gets infinite noise in the ranks past its own, whose
//    quotient is 0). top_k = 1 is the nearest thing to a greedy column. The setting belongs to the column, not the conversation: it survives
//    moshi_hot_slot_close / _open, and a newly opened slot restarts at frame 0 of its seed, so the same seed replays the same conversation.
//  * single-stream (b = 0): only the seed is free - temp, temp_text, top_k and top_k_text must equal the configuration's (its graphs keep them baked in).
//    Supported on the moshika-shaped LM (with or without the codec) stepped by moshi_hot_lm_step, moshi_hot_lm_step_n, moshi_hot_sts_frame and the
//    moshi_hot_sts_pipeline_* calls with chain_depth = 0, and on the stt-shaped LM (dep_q == 0: site 0 is its only sampler; extra heads allowed).
//    Returns -1 with chain_depth > 0 (moshi_hot_lm_step_run_ahead included), personaplex, extra heads on a model with a Depth transformer, demux, low-rank embeddings, delay_steps, cross-attention, condition_sum, a weight schedule, a Depth shard, a Depth hook or a tensor-parallel
//    stack. The text sample moshi_hot_lm_step_embedding computes and discards still draws from rand().
// A column that was never set draws from rand() exactly as before: the sweep over the whole noise tensor is always drawn in full, in the same order, and
// the rows of seeded columns are overwritten afterwards. A seeded column that is closed gets constant noise; its results are dropped.
GGML_API int moshi_hot_set_sampling(moshi_hot_model_t * m, int b, const struct moshi_hot_sampling * s);
// column b's current values (the configuration's until set; seed 0) and whether it has been seeded; -1 for a bad column
GGML_API int moshi_hot_get_sampling(moshi_hot_model_t * m, int b, struct moshi_hot_sampling * s, int * seeded);
// noise(seed, frame, site, rank) for rank = 0 .. n - 1 with lambd = 1 (tests)
GGML_API void moshi_hot_sampling_noise(uint64_t seed, int64_t frame, int site, int n, float * out);

// mimi_encode_send + mimi_encode_receive (src/moshi.cpp:215-234): 1920 samples -> mimi_n_q codes
GGML_API void moshi_hot_mimi_encode(moshi_hot_model_t * m, const float * pcm, int32_t * codes);
// mimi_decode_send + mimi_decode_receive (src/moshi.cpp:273-292): mimi_n_q codes -> 1920 samples
GGML_API void moshi_hot_mimi_decode(moshi_hot_model_t * m, const int32_t * codes, float * pcm);
// moshi_lm_send2 + moshi_lm_receive (src/moshi.cpp:904-926) = one moshi_lmgen_step (lm.h:778-979):
// in_audio = the (n_q - dep_q) codes of the other speaker; returns 1 when text/out_audio are valid
GGML_API int moshi_hot_lm_step(moshi_hot_model_t * m, const int32_t * in_audio, int32_t * text_token, int32_t * out_audio);
// moshi_lmgen_step in full (lm.h:778-979). n_tokens == n_q + 1: "provided" mode — every codebook of this frame is given (text first),
// the model still steps but its samples are not written to the delay ring: PersonaPlex prompt frames (lm.h:1063-1075, 1088-1097).
// Otherwise tokens = the other speaker's (n_q - dep_q) codes as in moshi_hot_lm_step. vad (may be NULL): softmax(extra_heads[2]·transformer_out)[0].
GGML_API int moshi_hot_lm_step_n(moshi_hot_model_t * m, const int32_t * tokens, int n_tokens, int32_t * text_token, int32_t * out_audio, float * vad);
// The LM step alone under run-ahead (config.chain_depth = 2; the codec-free half of moshi_hot_sts_pipeline_frame): queues the step of in_audio behind
// the previous one and returns the PREVIOUS step's result (1 / 0 like moshi_hot_lm_step, -1 when there is none yet). in_audio = NULL drains the last step.
GGML_API int moshi_hot_lm_step_run_ahead(moshi_hot_model_t * m, const int32_t * in_audio, int32_t * text_token, int32_t * out_audio);
// tts conditions: sum F32[dim] (may be NULL) and cross F32[dim * cross_len] (may be NULL); the cross-attention K/V of every layer are
// computed once here (init(), transformer.h:343-396). Call before the first step.
GGML_API void moshi_hot_set_conditions(moshi_hot_model_t * m, const float * sum, const float * cross);
// on_text_hook (lm.h:880-900): replaces the sampled text token (the TTS state machine lives above this boundary)
typedef int32_t (*moshi_hot_text_hook_t)(void * user, int64_t offset, int32_t sampled);
GGML_API void moshi_hot_set_text_hook(moshi_hot_model_t * m, moshi_hot_text_hook_t hook, void * user);
// one voice-prompt frame from a precomputed input embedding F32[dim] (moshi_lmgen_step_voice_prompt, lm.h:1004-1037): the Temporal
// stack runs on the scratch context (moshi_lmmodel_forward_embedding, lm.h:694-709), text is forced to 3, the Depth graph steps
GGML_API void moshi_hot_lm_step_embedding(moshi_hot_model_t * m, const float * embedding);
// n_frames provided frames (tokens: n_frames x (n_q + 1), text first) as batched [dim, T] passes of at most `chunk` frames (0 = 64, the largest the batched kernels take):
// leaves the delay ring, the offsets and the Temporal KV ring as n_frames calls of moshi_hot_lm_step_n(.., n_q + 1, ..) would,
// without running the Depth graph or the text head
GGML_API void moshi_hot_prefill(moshi_hot_model_t * m, const int32_t * tokens, int n_frames, int chunk);
// PROMPT_TOKENS (lm.h:983-987): 17 ids, text first
GGML_API const int32_t * moshi_hot_personaplex_prompt_tokens(void);
// moshi_lmgen_step_system_prompts without a voice (lm.h:1118-1134): 6 silence frames, the text prompt, 6 silence frames
GGML_API void moshi_hot_personaplex_system_prompts(moshi_hot_model_t * m, const int32_t * text_prompt, int n_text);
// the same 12 + n_text prompt frames as batched passes (moshi_hot_prefill): same state afterwards
GGML_API void moshi_hot_personaplex_system_prompts_batched(moshi_hot_model_t * m, const int32_t * text_prompt, int n_text, int chunk);
// one iteration of the moshi-sts --bench loop (tools/moshi-sts.cpp:770-808); returns 1 when a frame was produced
GGML_API int moshi_hot_sts_frame(moshi_hot_model_t * m, const float * pcm_in, int32_t * text_token, int32_t * audio_tokens, float * pcm_out);

// The moshi-sts --bench loop software-pipelined (tools/moshi-sts.cpp:770-808 feeds every frame without waiting for playback): the LM step of
// frame k runs on the backend's stream while the codec stream (config.codec_stream) decodes frame k - 1 and encodes frame k + 1. begin: encodes
// frame 0. frame: pcm_next = input of frame k + 1 (NULL: none follows); returns bit 0 = text_token / audio_tokens are valid, bit 1 = pcm_prev holds
// the output of frame k - 1, bit 2 = run-ahead (chain_depth = 2): the tokens are frame k - 1's too, because the LM step of frame k was queued behind
// the previous one before the host looked at that one's tokens (they reach the next Temporal graph through device memory; the LM stream never waits
// for the host). end: finishes what is outstanding: bit 0 = tokens of the last frame (run-ahead only), bit 1 = pcm_last is the last frame's output.
// Tokens and PCM are bit-identical to moshi_hot_sts_frame's: every graph consumes the same inputs and states in the same order.
GGML_API void moshi_hot_sts_pipeline_begin(moshi_hot_model_t * m, const float * pcm0);
GGML_API int  moshi_hot_sts_pipeline_frame(moshi_hot_model_t * m, const float * pcm_next, int32_t * text_token, int32_t * audio_tokens, float * pcm_prev);
GGML_API int  moshi_hot_sts_pipeline_end(moshi_hot_model_t * m, int32_t * text_token, int32_t * audio_tokens, float * pcm_last);
// stt / tts shaped models run the same loop with the codec half they have (encode of frame k + 1, or decode of frame k - 1, beside the LM step of frame k);
// the VAD head's probability of the last stepped frame (lm.h:966-976) is read here
GGML_API float moshi_hot_sts_pipeline_vad(moshi_hot_model_t * m);

// introspection for tests / bench
GGML_API int64_t moshi_hot_offset(moshi_hot_model_t * m);                      // frames stepped so far
GGML_API void    moshi_hot_last_raw_tokens(moshi_hot_model_t * m, int32_t * text_token, int32_t * audio_tokens);  // sampled this step, before the delay ring
GGML_API size_t  moshi_hot_weight_bytes(moshi_hot_model_t * m, int part);     // 0 temporal, 1 depth, 2 mimi enc, 3 mimi dec, 4 embeddings, 5 tensor-parallel slices (a subset of 0)
GGML_API int     moshi_hot_read_last(moshi_hot_model_t * m, const char * what, float * out, int64_t n);  // "text_logits", "transformer_out", "transformer_in", "stack_out", "dep_logits<k>", "enc_latent_first" / "enc_latent_rest" (F32[256]: what the RVQ stacks quantise)
// a weight tensor by its checkpoint-style name (e.g. "lm.transformer.layers.0.self_attn.in_projs.weight"); tests/ref_link uses it
// to hand the SAME tensors to the reference's own graph builders
GGML_API struct ggml_tensor * moshi_hot_weight(moshi_hot_model_t * m, const char * name);
// the cached graph of a phase once it has run (0 temporal, 1 depth, 2 mimi encoder, 3 mimi decoder), for structural comparison
GGML_API struct ggml_cgraph * moshi_hot_graph(moshi_hot_model_t * m, int which);
// per-phase wall clock (synchronises around each phase while on): us_per_call[4] = mimi encode, temporal, depth, mimi decode
GGML_API void    moshi_hot_set_timing(moshi_hot_model_t * m, int on);
GGML_API void    moshi_hot_get_timing(moshi_hot_model_t * m, double * us_per_call);
// teacher forcing for parity runs: overwrite the tokens the last moshi_hot_lm_step wrote into the delay ring
GGML_API void    moshi_hot_force_last(moshi_hot_model_t * m, int32_t text_token, const int32_t * audio_tokens);
GGML_API void    moshi_hot_set_context_fill(moshi_hot_model_t * m, int64_t offset); // jump the Temporal ring to a given fill level (bench only); on a single-stream codec-only model (enable_lm = 0): the codec transformers' positions, in frames (2 ring rows each)
// write the same pseudo-random BF16 rows (approximately N(0, scale^2), a function of seed / which / layer / position only) into EVERY slot of the K and V
// rings (transformer.h:156-172) of one layer (layer >= 0) or of all layers (-1) of the Temporal (which = 0) or Depth (1) transformer: two executors
// filled alike hold identical caches, so attention over hundreds or thousands of live slots can be compared node by node (tests only)
GGML_API void    moshi_hot_fill_ring(moshi_hot_model_t * m, int which, int layer, uint64_t seed, float scale);
// the reference's checkpoint path end to end (src/loader.h:85-99, 227-271): write every weight tensor of a model to a GGUF file / build a model whose
// weights are read back from such a file (names, types and sizes checked against the configuration) instead of being generated
GGML_API int     moshi_hot_save_gguf(moshi_hot_model_t * m, const char * path);
GGML_API moshi_hot_model_t * moshi_hot_create_from_gguf(ggml_backend_t backend, const struct moshi_hot_config * cfg, const char * path);
// the name a checkpoint tensor carries inside a GGUF file (WeightLoader::tensor_name, src/loader.h:120-137): the name itself below GGML_MAX_NAME characters,
// else the reference's 8-character CRC digest (src/crc-bbf.h). out receives at most n - 1 characters + NUL; returns the length of the file name
GGML_API int     moshi_hot_tensor_file_name(const char * checkpoint_name, char * out, int n);
// test hook: the host-side delay ring (rows x (n_q + 1) int32, row-major) -> dst; returns the value count (dst NULL: just the count)
GGML_API int     moshi_hot_host_ring(moshi_hot_model_t * m, int32_t * dst, int max_values);
// the inverse: the host-side delay ring <- rows (n_values = moshi_hot_host_ring's count), the frame count unchanged: what a single-stream model needs to
// take a voice's ring image (lm.h:1038-1052). Single-stream only. Returns 0, or -1 (nothing changes) on a B > 1 model or for another count.
GGML_API int     moshi_hot_set_host_ring(moshi_hot_model_t * m, const int32_t * rows, int n_values);
// the K (kv = 0) / V (kv = 1) ring of one layer as its bytes (BF16 [D, C, H]), read out (write = 0) or overwritten (write = 1): parity runs that restart every
// frame from another executor's state. Returns the ring's size in bytes (-1: no such ring); buf may be NULL to ask for the size. which: 0 Temporal, 1 Depth.
GGML_API int64_t moshi_hot_ring_bytes(moshi_hot_model_t * m, int which, int layer, int kv, void * buf, int64_t nbytes, int write);
// Parity probe: ONE transformer layer (moshi_streaming_transformer_layer, transformer.h:910-1039) of the Temporal (which = 0) or Depth
// (which = 1, with weight set `weight_set`) stack on the scratch context, fed x_in F32[dim] at stream position `offset` (mask row, RoPE
// phase and ring slot as transformer.h:1182-1215 computes them), over the model's own weights and KV ring of that layer (the new K / V
// rows are written at slot offset % capacity). Every tensor of the graph buffer is poisoned with 0xFF bytes before the compute, so a node
// a backend never materialised (fused away) reads back as NaN. After the compute `visit` is called for every node in execution order while
// the buffer is still alive (read values with ggml_backend_tensor_get); x_out (may be NULL) receives the layer output. Returns the node count.
typedef void (*moshi_hot_node_visitor_t)(void * user, int index, struct ggml_tensor * node);
GGML_API int     moshi_hot_layer_probe(moshi_hot_model_t * m, int which, int layer, int weight_set, const float * x_in, int offset, float * x_out,
                                       moshi_hot_node_visitor_t visit, void * user);

// ---- Depth codebook shard: one frame = begin, then for k = 0 .. dep_q-1 the owner runs `step` and everybody else `import` ---------------
// The 8-slot Depth ring is REPLICATED on every rank; what an owner hands on per step is one message of dep_layers * dep_dim + 8 32-bit words:
// its new K and V ring rows of all layers as the BF16 values the ring stores (2 * dep_layers * dep_dim of them: 24 KB at 6 x 1024) and, in the tail,
// the sampled token as F32 (+ the frame's stop flag in word 1 of the tail).
// The transport between ranks is the caller's (torch.distributed over RCCL / xGMI in bench.py, gloo in the CPU test): the message lives in
// one tensor whose storage pointer is returned here - a device pointer on the MI355X backend - so it can be handed to a collective as is.
GGML_API void *  moshi_hot_depth_shard_msg(moshi_hot_model_t * m, int64_t * n_floats);        // step message (rows + token)
GGML_API void *  moshi_hot_depth_shard_tout(moshi_hot_model_t * m, int64_t * n_floats);       // frame message: transformer_out F32[dim] + 8 (word dim = 1 while frames follow)
GGML_API void    moshi_hot_depth_shard_begin_export(moshi_hot_model_t * m, int32_t text_token, int more);   // Temporal owner: pack the frame message; text token feeds step 0
GGML_API int     moshi_hot_depth_shard_begin_import(moshi_hot_model_t * m);                   // others: unpack it; returns the "more frames" flag
GGML_API void    moshi_hot_depth_shard_step(moshi_hot_model_t * m, int k);                    // owner of step k: one Depth step (lm.h:505-527 body) + pack the message
GGML_API void    moshi_hot_depth_shard_import(moshi_hot_model_t * m, int k);                  // non-owner: rows -> ring slot k % capacity, token -> token vector
GGML_API void    moshi_hot_depth_shard_tokens(moshi_hot_model_t * m, int32_t * out, int n);   // the frame's sampled tokens so far
// The whole sharded frame behind the C-ABI - no interpreter on the critical path: the per-step loop above (owner: step + broadcast, the others: broadcast
// + import) runs inside these calls, the broadcasts go through ONE transport:
//   * RCCL, called from here (librccl.so is opened at run time; the harness links no HIP): ncclBroadcast on the backend's own HIP stream
//     (ggml_backend_mi355x_get_stream), i.e. stream-ordered behind the step's kernels and in front of the next ones - no host synchronisation and no
//     event per hop. Rank 0 makes the 128-byte unique id, the caller carries it to the other ranks (any side channel), every rank calls _rccl_init.
//   * or a caller-supplied function (host memory on the CPU device: gloo in tests/test_depth_shard_cpu.py; also a bring-up aid on devices).
typedef void (*moshi_hot_bcast_t)(void * user, void * data, int64_t bytes, int root);
GGML_API void    moshi_hot_depth_shard_set_transport(moshi_hot_model_t * m, moshi_hot_bcast_t fn, void * user);
GGML_API int     moshi_hot_depth_shard_rccl_unique_id(char * id128);                                            // 0 = ok (rank 0)
// _rccl_init makes the model's backend device current on the calling thread before ncclCommInitRank (the communicator binds to the current device) and
// replaces a communicator an earlier call made; the broadcasts / all-reduces return RCCL's code through GGML_ASSERT (a failed collective is not recoverable here).
GGML_API int     moshi_hot_depth_shard_rccl_init(moshi_hot_model_t * m, int rank, int world, const char * id128); // 0 = ok; every rank, collectively
GGML_API void    moshi_hot_depth_shard_rccl_free(moshi_hot_model_t * m);
GGML_API void    moshi_hot_depth_shard_broadcast(moshi_hot_model_t * m, int which, int root);                    // one broadcast of the step (0) / frame (1) message through the transport (latency probes)
// Temporal owner (rank 0): installs the sharded frame as the Depth half of moshi_hot_lm_step_n (export, broadcast, dep_q hops, read the tokens)
GGML_API void    moshi_hot_depth_shard_install(moshi_hot_model_t * m);
GGML_API void    moshi_hot_depth_shard_stop(moshi_hot_model_t * m);                                            // rank 0: tells the other ranks' _serve to return
GGML_API int64_t moshi_hot_depth_shard_hops(moshi_hot_model_t * m);                                            // broadcasts this rank has taken part in so far
GGML_API int64_t moshi_hot_depth_shard_serve(moshi_hot_model_t * m);                                           // every other rank: frames served until rank 0 stops
// ---- tensor-parallel Temporal stack: begin(x) ; for i in 0 .. 2 L: { segment(i) ; [i < 2 L: all-reduce(sum) of the message over the ranks] } ; end(out) ----
// segment 2 l   : x += message (l > 0) ; message = out_proj_r(attention_r(in_proj_r(norm1(x))))      (this rank's heads, its KV ring shard)
// segment 2 l+1 : x += message         ; message = linear_out_r(silu * mul of linear_in_r(norm2(x)))  (this rank's F / N hidden units)
// segment 2 L   : x += message         (the stack output)
GGML_API void *  moshi_hot_tp_msg(moshi_hot_model_t * m, int64_t * n_floats);          // the partial F32[dim] (device / host pointer: hand it to the collective)
GGML_API void    moshi_hot_tp_begin(moshi_hot_model_t * m, const float * x);            // stack input F32[dim]; advances the stream position (mask row, RoPE phase, ring slot)
GGML_API void    moshi_hot_tp_segment(moshi_hot_model_t * m, int i);
GGML_API void    moshi_hot_tp_end(moshi_hot_model_t * m, float * out);                  // stack output F32[dim]
// the same loop behind the C-ABI: every segment and the all-reduce (sum) of the partial between two of them - ncclAllReduce on the backend's stream through
// the model's communicator (moshi_hot_depth_shard_rccl_init), or a caller-supplied function over host memory (set_transport; CPU device / gloo tests)
typedef void (*moshi_hot_allreduce_t)(void * user, float * data, int64_t n_floats);
GGML_API void    moshi_hot_tp_set_transport(moshi_hot_model_t * m, moshi_hot_allreduce_t fn, void * user);
GGML_API void    moshi_hot_tp_stack(moshi_hot_model_t * m, const float * x, float * out);
GGML_API int64_t moshi_hot_tp_reductions(moshi_hot_model_t * m);
// The tensor-parallel stack as a FRAME mode (bench.py --shard temporal): on rank 0, after _install, the Temporal half of every moshi_hot_lm_step* is
//   embedding-sum graph -> broadcast of x (F32[dim] + a "more frames" flag; ncclBroadcast on the backend's stream, or the function of
//   moshi_hot_depth_shard_set_transport) -> the 2 L + 1 segments with their 2 L all-reduces -> out_norm / text head / sampler graph,
// and the Depth graph follows on rank 0 as in any LM step (lm.h:555-607, 659-677 around transformer.h:910-971). Every other rank sits in _serve: it takes the
// broadcast, runs its segments and joins the all-reduces until rank 0 calls _stop. Models are created with tp_world = N (>= 1), tp_rank, chain_depth = 0.
GGML_API void    moshi_hot_tp_install(moshi_hot_model_t * m);
GGML_API int64_t moshi_hot_tp_serve(moshi_hot_model_t * m);     // returns the frames served
GGML_API void    moshi_hot_tp_stop(moshi_hot_model_t * m);
GGML_API int64_t moshi_hot_tp_frames(moshi_hot_model_t * m);    // stack passes this rank has run in frame mode
GGML_API void    moshi_hot_tp_msg_read(moshi_hot_model_t * m, float * out);        // the partial-sum message, host copy out / in: lets ONE process sum the
GGML_API void    moshi_hot_tp_msg_write(moshi_hot_model_t * m, const float * in);   // partials of several ranks' models (tests without a second GPU)
// replaces the local chained Depth graph inside moshi_hot_lm_step_n: fn(user, text_token, audio[dep_q]) must fill all dep_q tokens
typedef void (*moshi_hot_depth_hook_t)(void * user, int32_t text_token, int32_t * audio);
GGML_API void    moshi_hot_set_depth_hook(moshi_hot_model_t * m, moshi_hot_depth_hook_t fn, void * user);

#ifdef __cplusplus
}
#endif
