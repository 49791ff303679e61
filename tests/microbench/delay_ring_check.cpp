// Stand-alone check of csrc/delay_ring.h (host code only, no GPU): random protocols and frame sequences - provided frames, other speaker's codes,
// commits with and without the run-ahead exception, forced frames - against the vector-of-rows arithmetic the driver used before DelayRing. Build and
// run under the sanitizers:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Imoshi.cpp_amd/csrc tests/microbench/delay_ring_check.cpp -o delay_ring_check && ./delay_ring_check
#include "delay_ring.h"
#include <stdio.h>
#include <stdlib.h>
int main() {
    srand(1);
    for (int trial = 0; trial < 200; trial++) {
        DelayProtocol p;
        const bool pp = trial % 3 == 0;
        p.n_q = pp ? 16 : 2 + rand() % 8; p.dep_q = pp ? 16 : rand() % (p.n_q + 1); p.io_dep_q = pp ? 8 : p.dep_q;
        for (int i = 0; i <= p.n_q; i++) { p.delays.push_back(rand() % 4); if (p.delays[i] > p.max_delay) p.max_delay = p.delays[i]; }
        p.rows = p.max_delay + 2 + pp; p.initial.assign(p.n_q + 1, 64); p.initial[0] = 500;
        DelayRing r; r.p = &p; r.reset();
        const int ncb = p.n_q + 1, CT = p.rows, dq1 = p.io_dep_q + 1, needed = ncb - dq1;
        std::vector<std::vector<int>> cache(CT, std::vector<int>(ncb, -2)); int offset = 0;
        for (int f = 0; f < 40; f++) {
            std::vector<int32_t> tok(ncb), audio(p.dep_q), audio2;
            for (auto & t : tok) t = rand() % 64 - 1;
            for (auto & a : audio) a = rand() % 64 - 1;
            const bool provided = needed > 0 && rand() % 4 == 0, keep = rand() % 5 == 0;
            if (provided) { r.feed_provided(tok.data()); for (int i = 0; i < ncb; i++) cache[(offset + p.delays[i]) % CT][i] = tok[i]; }
            else if (needed > 0) { r.feed_user(tok.data(), r.frames); for (int i = 0; i < needed; i++) cache[(offset + p.delays[dq1 + i]) % CT][dq1 + i] = tok[i]; }
            for (int i = 0; i < ncb; i++) { int want = offset <= p.delays[i] ? p.initial[i] : cache[offset % CT][i]; if (r.input(i, r.frames) != want) { printf("input mismatch\n"); return 1; } }
            const int text = rand() % 500;
            r.commit(text, audio.data(), provided, keep);
            offset++;
            if (!provided) { cache[offset % CT][0] = text; for (int q = 0; q < p.dep_q; q++) { if (keep && q + 1 >= dq1 && p.delays[q + 1] == 0) continue; cache[offset % CT][q + 1] = audio[q]; } }
            audio2 = audio; int32_t t1 = -9, t2 = -9; int ok2 = -1;
            if (offset > p.max_delay) { t2 = cache[(offset - p.max_delay + p.delays[0]) % CT][0]; for (int i = 1; i < dq1; i++) audio2[i - 1] = cache[(offset - p.max_delay + p.delays[i]) % CT][i]; ok2 = 1; for (int x : audio2) if (x == -1) ok2 = 0; }
            const DelayRing::ReadOut ro = r.read_out(&t1, audio.data());
            const int ok1 = ro == DelayRing::ReadOut::filling ? -1 : ro == DelayRing::ReadOut::valid ? 1 : 0;
            if (ok1 != ok2 || t1 != t2 || audio != audio2) { printf("read_out mismatch trial %d frame %d\n", trial, f); return 1; }
            if (rand() % 3 == 0) { for (auto & a : audio) a = rand() % 64; r.force_last(7, audio.data()); cache[offset % CT][0] = 7; for (int q = 0; q < p.dep_q; q++) cache[offset % CT][q + 1] = audio[q]; }
            std::vector<int32_t> flat(r.rows.size()); r.export_rows(flat.data());
            for (int a = 0; a < CT; a++) for (int b = 0; b < ncb; b++) if (flat[a * ncb + b] != cache[a][b]) { printf("ring mismatch\n"); return 1; }
            if (r.frames != offset) return 1;
        }
    }
    printf("delay_ring ok\n");
    return 0;
}
