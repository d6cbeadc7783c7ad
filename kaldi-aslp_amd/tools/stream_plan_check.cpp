// stream_plan_check.cpp -- the batch plans of nnet/stream-batch-plan.h against the host loops they restate (SequenceDataReader::FillBatchBuff
// and the chunk assembly of the latency-controlled tools), on random stream states: utterances shorter than the delay, streams that never
// received one, the rewind by the right context, every skip offset.  Host only and with a main of its own, so that the index arithmetic can
// run under the sanitizers:  make -C kaldi-aslp_amd plancheck   (g++ -fsanitize=address,undefined).  Every planned source row is also
// bounds-checked against the utterance it points into, which is what the gather on the device relies on.
#include <cstdio>
#include <random>

#include "stream-batch-plan.h"

using namespace aslp;

static int g_fail = 0;
#define CHECK(cond)                                                                   \
  do {                                                                                \
    if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); g_fail++; } \
  } while (0)

struct Utt { std::vector<float> feats; std::vector<int32> tgt; int32 rows; };   // one column: the frame's own number, the target 1000 + it

static Utt MakeUtt(int32 rows) {
  Utt u;
  u.rows = rows;
  for (int32 i = 0; i < rows; i++) { u.feats.push_back((float)i); u.tgt.push_back(1000 + i); }
  return u;
}

// what the plan means, carried out on the host: the batch's one feature column and the targets (-1: none)
static void Apply(const StreamBatchPlan &p, const std::vector<Utt> &utt, const std::vector<std::vector<int32>> &tgt, int32 S,
                  std::vector<float> *x, std::vector<int32> *t) {
  x->assign(p.src_frame.size(), 0.0f);
  t->assign(p.src_frame.size(), -1);
  for (size_t row = 0; row < p.src_frame.size(); row++) {
    const int32 s = (int32)(row % S), f = p.src_frame[row], i = p.tgt_index[row];
    CHECK(f >= -1 && f < utt[s].rows);
    CHECK(i >= -1 && i < (int32)tgt[s].size());
    if (f >= 0 && f < utt[s].rows) (*x)[row] = utt[s].feats[f];
    if (i >= 0 && i < (int32)tgt[s].size()) (*t)[row] = tgt[s][i];
  }
}

static void CheckSequence(std::mt19937 &rng) {
  const int32 S = 1 + rng() % 6, B = 1 + rng() % 7, delay = rng() % 5, w = 1 + rng() % 3, off = w > 1 ? rng() % w : 0;
  std::vector<Utt> utt(S);
  std::vector<std::vector<float>> feats(S);    // the host reader's thinned copies
  std::vector<std::vector<int32>> tgt(S);
  std::vector<int32> curt(S, 0), lent(S, 0);
  for (int32 s = 0; s < S; s++) {
    utt[s] = MakeUtt(rng() % 4 == 0 ? 0 : 1 + rng() % 12);    // 0 rows: the stream never received an utterance
    const int32 rows = utt[s].rows;
    const int32 len = w > 1 ? (rows > off ? (rows - 1 - off) / w + 1 : 0) : rows;
    for (int32 i = 0; i < len; i++) {
      const int32 src = w > 1 ? i * w + off : i;
      feats[s].push_back(utt[s].feats[src]);
      tgt[s].push_back(utt[s].tgt[src]);
    }
    lent[s] = len;
  }
  for (int step = 0; step < 6; step++) {
    std::vector<int32> c2 = curt;
    StreamBatchPlan plan;
    PlanSequenceBatch(B, delay, w, off, &c2, lent, &plan);
    // data-reader.h, FillBatchBuff
    bool done = true;
    for (int32 s = 0; s < S; s++) if (curt[s] < lent[s]) done = false;
    CHECK(plan.all_done == done);
    std::vector<float> x((size_t)B * S, 0.0f), mask((size_t)B * S, 0.0f);
    std::vector<int32> t((size_t)B * S, -1);
    if (!done) {
      for (int32 tt = 0; tt < B; tt++) {
        for (int32 s = 0; s < S; s++) {
          const size_t row = (size_t)tt * S + s;
          if (lent[s] == 0) { curt[s]++; continue; }
          if (curt[s] < lent[s]) { mask[row] = 1.0f; t[row] = tgt[s][curt[s]]; }
          else t[row] = tgt[s][lent[s] - 1];
          const int32 src = curt[s] + delay < lent[s] ? curt[s] + delay : lent[s] - 1;
          x[row] = feats[s][src];
          curt[s]++;
        }
      }
    }
    std::vector<float> px;
    std::vector<int32> pt;
    Apply(plan, utt, tgt, S, &px, &pt);
    CHECK(px == x);
    CHECK(pt == t);
    CHECK(plan.mask == mask);
    CHECK(c2 == curt);
  }
}

static void CheckChunk(std::mt19937 &rng) {
  const int32 S = 1 + rng() % 6, chunk = 1 + rng() % 6, right = rng() % 4, B = chunk + right;
  std::vector<Utt> utt(S);
  std::vector<std::vector<int32>> tgt(S);
  std::vector<int32> curt(S, 0), lent(S, 0);
  for (int32 s = 0; s < S; s++) {
    utt[s] = MakeUtt(rng() % 4 == 0 ? 0 : 1 + rng() % 20);
    tgt[s] = utt[s].tgt;
    lent[s] = utt[s].rows;
  }
  for (int step = 0; step < 8; step++) {
    std::vector<int32> c2 = curt;
    StreamBatchPlan plan;
    PlanChunkBatch(chunk, right, &c2, lent, &plan);
    bool done = true;
    for (int32 s = 0; s < S; s++) if (curt[s] < lent[s]) done = false;
    CHECK(plan.all_done == done);
    if (done) { CHECK(c2 == curt); continue; }
    // tools/stream_tools.cpp, the chunk assembly as it stood on the host
    std::vector<float> x((size_t)B * S, 0.0f), mask((size_t)B * S, 0.0f);
    std::vector<int32> t((size_t)B * S, -1);
    for (int32 tt = 0; tt < B; tt++) {
      for (int32 s = 0; s < S; s++) {
        const size_t row = (size_t)tt * S + s;
        if (curt[s] < lent[s]) {
          mask[row] = tt >= chunk ? 0.0f : 1.0f;
          t[row] = tgt[s][curt[s]];
          x[row] = utt[s].feats[curt[s]];
        } else {
          if (lent[s] > 0) t[row] = tgt[s][lent[s] - 1];
        }
        curt[s]++;
      }
    }
    for (int32 s = 0; s < S; s++) curt[s] -= right;
    std::vector<float> px;
    std::vector<int32> pt;
    Apply(plan, utt, tgt, S, &px, &pt);
    CHECK(px == x);
    CHECK(pt == t);
    CHECK(plan.mask == mask);
    CHECK(c2 == curt);
  }
}

int main() {
  std::mt19937 rng(12345);
  for (int i = 0; i < 4000; i++) { CheckSequence(rng); CheckChunk(rng); }
  if (g_fail) { std::printf("stream_plan_check: %d checks FAILED\n", g_fail); return 1; }
  std::printf("stream_plan_check: ok\n");
  return 0;
}
