// delay_ring.h — the host half of moshi_lmgen_step (lm.h:778-979) as one type: the delay ring of moshi_lmgen_state (lm.h:715-743) and every read
// and write the frame protocol makes on it. A single-stream model holds one DelayRing, a B > 1 model one per column; nothing else indexes a ring.
// Plain C++ (no ggml): the integer protocol can be compiled and tested on its own.
#pragma once
#include <stdint.h>
#include <string.h>
#include <vector>

// moshi_lmmodel_text_token_embed_step (lm.h:586-607): what an id becomes as an embedding input: -1 -> scale 0, negative ids -> row 0
struct TokenInput { int32_t row; float scale; };
inline TokenInput token_input(int32_t id) { return { id < 0 ? 0 : id, id == -1 ? 0.f : 1.f }; }

// What a configuration fixes of the protocol: bound once at model creation, shared by every ring of the model
struct DelayProtocol {
    std::vector<int> delays, initial;   // per column (text, then the n_q codebooks): its delay, and the token fed until the ring has one (lm.h:722-743)
    int max_delay = 0, n_q = 0, rows = 0;   // rows: of the ring (lm.h:727-731)
    int dep_q = 0, io_dep_q = 0;        // codebooks the model samples per frame; those of them the protocol hands back (PersonaPlex: 16 and 8, lm.h:802-805)
    int cols() const { return n_q + 1; }
    int needed() const { return n_q - io_dep_q; }   // the other speaker's codes a frame takes
};

struct DelayRing {
    const DelayProtocol * p = nullptr;
    std::vector<int32_t> rows;          // [p->rows][n_q + 1] row-major (moshi_hot_host_ring, the snapshot blob); -2: never written
    int64_t frames = 0;                 // frames stepped so far (moshi_lmgen_state's offset)
    enum class ReadOut { filling, gap, valid };

    void reset() { rows.assign((size_t) p->rows * (size_t) p->cols(), -2); frames = 0; }   // a fresh stream
    // a provided frame - every column given - enters the ring (lm.h:812-817)
    void feed_provided(const int32_t * tokens) { for (int i = 0; i < p->cols(); i++) cell(frames + p->delays[i], i) = tokens[i]; }
    // the other speaker's codes enter the ring at frame `at` (lm.h:819-824); at > frames: a step queued behind ones that are still running
    void feed_user(const int32_t * codes, int64_t at) {
        for (int i = p->io_dep_q + 1; i < p->cols(); i++) cell(at + p->delays[i], i) = codes[i - p->io_dep_q - 1];
    }
    // column i of the model's input row at frame `at` (lm.h:826-834)
    int32_t input(int i, int64_t at) const { return at <= p->delays[i] ? p->initial[(size_t) i] : rows[index(at, i)]; }
    // the frame is over (lm.h:933-943): the count advances and, unless the frame was provided, the model's samples go into the next frame's row.
    // keep_user_codes: a newer run-ahead step has already been queued and has put the other speaker's delay-0 codes into this very row; in the serial
    // order this write comes first and those codes land on top of it, so they stay
    void commit(int32_t text, const int32_t * audio, bool provided, bool keep_user_codes = false) {
        ++frames;
        if (!provided) force_last(text, audio, keep_user_codes);
    }
    // the delayed read-out (lm.h:950-964). audio holds the frame's dep_q raw samples; once the ring is full, *text and the first io_dep_q entries of
    // audio become the delayed tokens and the result tells whether a -1 is among all dep_q entries (PersonaPlex: the tail is still the raw samples)
    ReadOut read_out(int32_t * text, int32_t * audio) const {
        if (frames <= p->max_delay) return ReadOut::filling;
        *text = rows[index(frames - p->max_delay + p->delays[0], 0)];
        for (int i = 1; i <= p->io_dep_q; i++) audio[i - 1] = rows[index(frames - p->max_delay + p->delays[i], i)];
        for (int q = 0; q < p->dep_q; q++) if (audio[q] == -1) return ReadOut::gap;
        return ReadOut::valid;
    }
    // the model's samples of the last frame, written or (moshi_hot_force_last: teacher forcing) replaced
    void force_last(int32_t text, const int32_t * audio, bool keep_user_codes = false) {
        cell(frames, 0) = text;
        for (int q = 0; q < p->dep_q; q++)
            if (!(keep_user_codes && q >= p->io_dep_q && p->delays[q + 1] == 0)) cell(frames, q + 1) = audio[q];
    }
    int32_t last(int i) const { return rows[index(frames, i)]; }   // column i of the row the last frame committed
    void export_rows(int32_t * dst) const { memcpy(dst, rows.data(), rows.size() * sizeof(int32_t)); }
    void import_rows(const int32_t * src, int64_t frames_) { memcpy(rows.data(), src, rows.size() * sizeof(int32_t)); frames = frames_; }

private:
    size_t index(int64_t frame, int i) const { return (size_t) (frame % p->rows) * (size_t) p->cols() + (size_t) i; }
    int32_t & cell(int64_t frame, int i) { return rows[index(frame, i)]; }
};
