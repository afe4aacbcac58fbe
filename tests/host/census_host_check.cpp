// census_host_check.cpp -- the host code of score mode's census (clair3_amd/csrc/c3_census.h) without a device: plan_batch with and without
// the census section (the score section stays what it was), record_batch and the reader of a completed batch (read_score: the batch's table
// joins the handle's totals, once per batch, 32-bit counts widened to the 64-bit totals), and the three entries' refusals -- driven against
// plain host buffers that are exactly as large as the plan says, so that a byte read or written outside them is an error under
// AddressSanitizer.  Stand-alone, host only:
//
//   hipcc --offload-arch=gfx950 -x hip -std=c++20 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -DC3HIP_SRC_HASH='"host-check"' tests/host/census_host_check.cpp -o census_host_check && ./census_host_check
//
// (the library's one translation unit, so the device code is compiled along; it is not run.)  No HIP call is made and no device is needed:
// the slot's "pinned" buffers are malloc'ed here.
#include "../../clair3_amd/csrc/c3_model.hip"

#include <cstdio>
#include <random>

using namespace c3;

static int failures = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) ++failures, fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
    } while (0)

// a table as a kernel could have left it: counts up to the largest a batch can reach, every cell of a task the model has
static ScoreCensusTable random_table(const c3_model *m, std::mt19937 &rng, bool large) {
    ScoreCensusTable t = ScoreCensusTable{};
    const uint32_t top = large ? 0xffffffffu : 1000u;
    for (int h = 0; h < m->nb; ++h) {
        for (int i = 0; i < kScoreCensusClasses[h] * kScoreCensusClasses[h]; ++i) t.confusion[kScoreCensusCellOff[h] + i] = rng() % top;
        for (int b = 0; b < kScoreCensusBins; ++b) {
            t.rel_windows[h][b] = rng() % top, t.rel_correct[h][b] = rng() % top;
            t.rel_conf_q32[h][b] = large ? ((uint64_t)1 << 50) - rng() : (uint64_t)rng() << 8;  // (far beyond 32 bits; 80 batches stay inside int64)
        }
        t.rel_skipped[h] = rng() % top;
        for (int k = 0; k < kScoreCensusGaps; ++k) t.gap_below[h][k] = rng() % top;
    }
    return t;
}

static void one_batch(c3_model *m, int64_t batch, int label_dtype, bool want_rows, bool want_losses, bool verify, std::mt19937 &rng) {
    want_rows &= batch > 0, want_losses &= batch > 0;
    const size_t wbytes = (size_t)c3_model_window_bytes(m, C3_DTYPE_I8), lsize = label_dtype == C3_DTYPE_F32 ? 4 : 1;
    std::vector<uint8_t> x((size_t)batch * wbytes), labels((size_t)batch * m->nout * lsize);
    std::vector<float> y((size_t)batch * m->row, -1.f), losses((size_t)batch * m->nb, -1.f);
    RingInput in = ring_input(InKind::Sliced, x.data(), C3_DTYPE_I8, batch, want_rows ? y.data() : nullptr);
    in.score = true, in.labels = labels.data(), in.label_dtype = label_dtype, in.loss_host = want_losses ? losses.data() : nullptr;
    // off: the plan of the parent, no census section
    m->score_census_on = false;
    const StagedBatch off = plan_batch(m, in, false, verify, false);
    CHECK(off.census.bytes == 0 && off.census.off == 0);
    CHECK(off.y_total == (want_losses ? off.losses.off + off.losses.bytes : off.score.off + off.score.bytes));
    // on: everything in front of the new section is where it was; the section starts at a multiple of 256 bytes and ends the buffer
    m->score_census_on = true;
    const StagedBatch p = plan_batch(m, in, false, verify, false);
    CHECK(p.score.off == off.score.off && p.score.bytes == kScoreRecordBytes && p.losses.off == off.losses.off && p.losses.bytes == off.losses.bytes);
    CHECK(p.labels.off == off.labels.off && p.labels.bytes == off.labels.bytes && p.staged == off.staged && p.x_cap == off.x_cap);
    CHECK(p.y.bytes == off.y.bytes && p.verify.off == off.verify.off && p.verify.bytes == off.verify.bytes);
    CHECK(p.census.bytes == kScoreCensusBytes && p.census.bytes >= sizeof(ScoreCensusTable) && p.census.bytes % 256 == 0);
    CHECK(p.census.off % 256 == 0 && p.census.off >= off.y_total && p.census.off < off.y_total + 256 && p.y_total == p.census.off + p.census.bytes);
    // a batch that is not scored has no such section whatever the handle says
    RingInput plain = in;
    plain.score = false, plain.labels = nullptr, plain.loss_host = nullptr, plain.y_host = y.data();
    const StagedBatch q = plan_batch(m, plain, false, verify, false);
    CHECK(q.census.bytes == 0 && q.score.bytes == 0 && q.y_total == (verify ? q.verify.off + q.verify.bytes : q.y.bytes));

    // the reader: two batches through the same slot, each counted once
    HostSlot sl;
    std::vector<uint8_t> pin_x(p.x_cap), pin_y(p.y_total);
    sl.pin_x = pin_x.data(), sl.pin_y = (float *)pin_y.data();
    const c3_score_census before = m->score_census;
    c3_score_census want = before;
    for (int round = 0; round < 2; ++round) {
        record_batch(m, sl, in, p, -1);
        const ScoreCensusTable t = random_table(m, rng, round == 1);
        ScoreRecord rec = ScoreRecord{};
        rec.windows = (int32_t)batch, rec.tasks = m->nb;
        memcpy(pin_y.data() + p.score.off, &rec, sizeof(rec));
        memcpy(pin_y.data() + p.census.off, &t, sizeof(t));
        read_score(sl, m);
        CHECK(sl.score_rec.windows == batch);
        want.windows += batch, want.tasks = m->nb;
        for (int i = 0; i < kScoreCensusCells; ++i) want.confusion[i] += (int64_t)t.confusion[i];
        for (int h = 0; h < 4; ++h) {
            for (int b = 0; b < kScoreCensusBins; ++b) {
                want.rel_windows[h][b] += (int64_t)t.rel_windows[h][b], want.rel_correct[h][b] += (int64_t)t.rel_correct[h][b];
                want.rel_conf_q32[h][b] += (int64_t)t.rel_conf_q32[h][b];
            }
            want.rel_skipped[h] += (int64_t)t.rel_skipped[h];
            for (int k = 0; k < kScoreCensusGaps; ++k) want.gap_below[h][k] += (int64_t)t.gap_below[h][k];
        }
        CHECK(memcmp(&m->score_census, &want, sizeof(want)) == 0);
    }
    // the tables of tasks the model does not have stay zero
    for (int h = m->nb; h < 4; ++h) {
        for (int i = kScoreCensusCellOff[h]; i < kScoreCensusCellOff[h] + kScoreCensusClasses[h] * kScoreCensusClasses[h]; ++i) CHECK(m->score_census.confusion[i] == 0);
        CHECK(m->score_census.rel_skipped[h] == 0 && m->score_census.gap_below[h][5] == 0 && m->score_census.rel_conf_q32[h][19] == 0);
    }
    // a batch planned while the census was off adds nothing, and its reader touches nothing behind its own buffer
    std::vector<uint8_t> small_y(off.y_total);
    sl.pin_y = (float *)small_y.data();
    m->score_census_on = false;
    record_batch(m, sl, in, off, -1);
    read_score(sl, m);
    CHECK(memcmp(&m->score_census, &want, sizeof(want)) == 0);
    // the reader as score_host_check.cpp calls it: no handle, no accumulation
    sl.pin_y = (float *)pin_y.data();
    record_batch(m, sl, in, p, -1);
    read_score(sl);
    CHECK(memcmp(&m->score_census, &want, sizeof(want)) == 0);
}

static void entries(c3_model *m) {
    c3_score_census out;
    m->score_on = false, m->score_census_on = false, m->score_census_seen = false;
    CHECK(c3_model_set_score_census(nullptr, 1) != 0 && strstr(c3_last_error(), "null model"));
    CHECK(c3_score_census_read(nullptr, &out) != 0 && c3_score_census_reset(nullptr) != 0);
    CHECK(c3_model_set_score_census(m, 1) != 0 && strstr(c3_last_error(), "c3_model_set_score first"));
    CHECK(c3_score_census_read(m, &out) != 0 && strstr(c3_last_error(), "score mode is off"));
    m->score_on = true;
    CHECK(c3_score_census_read(m, &out) != 0 && strstr(c3_last_error(), "never enabled"));
    CHECK(c3_score_census_reset(m) != 0 && strstr(c3_last_error(), "never enabled"));
    m->slot[2].busy = true;
    CHECK(c3_model_set_score_census(m, 1) != 0 && strstr(c3_last_error(), "in flight") && !m->score_census_on);
    m->slot[2].busy = false;
    CHECK(c3_model_set_score_census(m, 1) == 0 && m->score_census_on && m->score_census_seen);
    CHECK(c3_score_census_read(m, nullptr) != 0 && strstr(c3_last_error(), "out"));
    CHECK(c3_score_census_read(m, &out) == 0 && out.windows == 0 && out.tasks == m->nb && out.confusion[0] == 0);
    m->score_census.windows = 5, m->score_census.confusion[2627] = 7, m->score_census.gap_below[3][5] = 9;
    CHECK(c3_model_set_score_census(m, 0) == 0 && !m->score_census_on);  // off: the totals stay readable
    CHECK(c3_score_census_read(m, &out) == 0 && out.windows == 5 && out.confusion[2627] == 7 && out.gap_below[3][5] == 9);
    CHECK(c3_model_set_score_census(m, 1) == 0 && m->score_census.windows == 5);  // on again: they go on
    CHECK(c3_score_census_reset(m) == 0 && c3_score_census_read(m, &out) == 0 && out.windows == 0 && out.confusion[2627] == 0 && out.tasks == m->nb);
    CHECK(sizeof(c3_score_census) == 23184);
}

int main() {
    std::mt19937 rng(12);
    c3_model *pileup = new c3_model(), *fa = new c3_model();
    pileup->kind = C3_KIND_PILEUP, pileup->C = 18, pileup->nb = 2, pileup->nout = 24, pileup->row = 24;
    fa->kind = C3_KIND_FULL_ALIGNMENT, fa->C = 9, fa->depth = 55, fa->nb = 4, fa->nout = 90, fa->row = 90 + kDecodeCols;  // (odd window and row sizes)
    for (c3_model *m : {pileup, fa}) {
        entries(m);
        for (int64_t batch : {0, 1, 3, 65, 257})
            for (int ld : {C3_DTYPE_I8, C3_DTYPE_F32})
                for (int mask = 0; mask < 8; ++mask) one_batch(m, batch, ld, mask & 1, mask & 2, mask & 4, rng);
    }
    delete pileup;
    delete fa;
    printf("census_host_check: %d failure(s)\n", failures);
    return failures != 0;
}
