// result_words_check — the tagged result words, their wait and the walks over them (csrc/result_words.hpp).
//
// Host only.  A writer thread plays the device and the other ranks: it stores the words a walk needs, in a chosen
// order, into heap blocks of exact size (so the sanitizers see a walk that reads a word it has no business with).
// Words nobody stores keep a stale tag and a value that would mislead a walk that ignored the tag.  Every walk
// is compared with a naive second implementation that sees all values at once: it flattens the candidates,
// sorts them by global index and takes the first drainable one.  Exits 1 on a mismatch, 2 when the random
// cases of a run missed one of the corners listed at the end of main().
//
//   result_words_check [cases] [seed]
#include <algorithm>
#include <atomic>
#include <chrono>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <thread>
#include <vector>

#include "../include/sr_planner.h"
#include "result_words.hpp"

using namespace sr;

namespace {

// The words before a mapping are an argument of the walks (kernels.hpp, which needs HIP, has the planner's
// kResultHeader = 8 and kPdbHeader = 2): the header and ledger checks run with those and with other counts.
constexpr int kHeader = 8;
constexpr int32_t kPending = 0, kFallback = SR_CAND_FALLBACK, kEmpty = SR_CAND_EMPTY;
const auto kLong = std::chrono::seconds(30);                  // a limit no healthy run reaches
const auto kShort = std::chrono::milliseconds(3);

std::mt19937 g_rng;
int pick(int lo, int hi) { return lo + static_cast<int>(g_rng() % static_cast<uint32_t>(hi - lo + 1)); }

std::atomic<int> g_failures{0};
#define CHECK(cond)                                                                        \
  do {                                                                                     \
    if (!(cond)) {                                                                         \
      std::fprintf(stderr, "result_words_check: line %d: %s\n", __LINE__, #cond);          \
      g_failures += 1;                                                                     \
      return false;                                                                        \
    }                                                                                      \
  } while (0)

using Block = std::unique_ptr<uint64_t[]>;
Block block(size_t n, uint64_t fill) {
  Block b(new uint64_t[n]);
  std::fill(b.get(), b.get() + n, fill);
  return b;
}

struct Store {
  volatile uint64_t* p;
  uint64_t v;
  bool held = false;  // the writer lets time pass before this store: a walk that does not wait for it is gone by then
};

// The device (or a peer): the stores in order from a thread of its own; joined when it leaves scope.
struct Writer {
  std::thread t;
  Writer(std::vector<Store> s, int delay_us, std::atomic<bool>* started = nullptr)
      : t([s = std::move(s), delay_us, started] {
          if (delay_us) std::this_thread::sleep_for(std::chrono::microseconds(delay_us));
          if (started) started->store(true);
          for (const Store& x : s) {
            if (x.held) std::this_thread::sleep_for(std::chrono::microseconds(100));
            *x.p = x.v;
            std::this_thread::yield();
          }
        }) {}
  ~Writer() { t.join(); }
};

// order: 0 all in place before the walk, 1 forward, 2 reverse, 3 shuffled (from the writer thread)
void arrange(std::vector<Store>* s, int order) {
  if (order == 2) std::reverse(s->begin(), s->end());
  if (order == 3) std::shuffle(s->begin(), s->end(), g_rng);
}
std::unique_ptr<Writer> deliver(std::vector<Store> s, int order) {
  arrange(&s, order);
  if (order == 0) {
    for (const Store& x : s) *x.p = x.v;
    return nullptr;
  }
  return std::make_unique<Writer>(std::move(s), pick(0, 2) ? 0 : pick(20, 200));
}

// The planner's stream fallback.
struct Spy {
  int calls = 0;
  bool ok = true;
  std::vector<Store> brings;  // what the stream wait finds written
};
bool spy_sync(void* user) {
  Spy* s = static_cast<Spy*>(user);
  s->calls += 1;
  for (const Store& x : s->brings) *x.p = x.v;
  return s->ok;
}

// A tag's stale relatives: the run before, fresh memory, the other transport's tag space.
uint64_t stale(uint32_t tag, uint32_t v) {
  const uint32_t t[3] = {tag - 1, 0u, tag ^ 0x80000000u};
  return word::make(t[pick(0, 2)], v);
}

// A mapping as a walk returned it, looked at the moment the walk returns, while the writer may still be storing:
// every word must already be this run's.  (Looked at after the writer is joined, a walk that came back before its
// mapping had arrived would pass.)
struct Seen {
  int32_t np = 0;
  bool ready = true;
  std::vector<int32_t> values;
  bool is(const std::vector<int32_t>& want) const { return ready && np == static_cast<int32_t>(want.size()) && values == want; }
};
Seen see(const volatile uint64_t* words, int32_t np, uint32_t tag, size_t at_most) {
  Seen g;
  g.np = np;
  const int32_t n = std::max(0, std::min(np, static_cast<int32_t>(at_most)));
  for (int32_t q = 0; q < n; ++q) g.ready = g.ready && word::ready(words + q, tag);
  g.values.resize(static_cast<size_t>(n));
  copy_values(words, n, g.values.data());
  return g;
}
// The stores of a mapping; the first two are held back, so the mapping arrives after the status word that
// names it and its second word after its first.
void map_stores(std::vector<Store>* s, volatile uint64_t* words, const std::vector<int32_t>& values, uint32_t tag) {
  for (size_t q = 0; q < values.size(); ++q)
    s->push_back({words + q, word::make(tag, static_cast<uint32_t>(values[q])), q < 2});
}

// ---- the wait
bool check_wait() {
  const uint32_t tag = 0x1234u;
  {  // present at entry; arrives before the limit
    Spy spy;
    ResultWait w(spy_sync, &spy, kLong, kLong);
    Block b = block(2, word::make(tag - 1, 1));
    b[0] = word::make(tag, 9);
    CHECK(w.own_word(b.get(), tag) == kWordsOk && word::value(b.get()) == 9);
    {
      Writer dev({{b.get() + 1, word::make(tag, 5)}}, 1000);
      CHECK(w.own_word(b.get() + 1, tag) == kWordsOk && word::value(b.get() + 1) == 5);
    }
    CHECK(spy.calls == 0 && !w.synced());
  }
  {  // never arrives: one stream wait, then "not written"; the next missing word fails without another
    Spy spy;
    ResultWait w(spy_sync, &spy, kShort, kLong);
    Block b = block(3, word::make(tag - 1, 1));
    b[2] = word::make(tag, 4);
    CHECK(w.own_word(b.get(), tag) == kWordsNotWritten && spy.calls == 1 && w.synced());
    CHECK(w.own_word(b.get() + 1, tag) == kWordsNotWritten && spy.calls == 1);
    CHECK(w.own_word(b.get() + 2, tag) == kWordsOk);  // (a word that is there still reads)
    CHECK(w.own_span(b.get(), 3, tag) == kWordsNotWritten && spy.calls == 1);
  }
  {  // a span whose words arrive one after the other: all of them are there when the wait returns
    Spy spy;
    ResultWait w(spy_sync, &spy, kLong, kLong);
    Block b = block(3, word::make(tag - 1, 1));
    Writer dev({{b.get(), word::make(tag, 1), true}, {b.get() + 1, word::make(tag, 2), true}, {b.get() + 2, word::make(tag, 3), true}}, 0);
    CHECK(w.own_span(b.get(), 3, tag) == kWordsOk && see(b.get(), 3, tag, 3).is({1, 2, 3}) && spy.calls == 0);
  }
  {  // the stream wait itself finds the word written
    Spy spy;
    Block b = block(1, 0);
    spy.brings = {{b.get(), word::make(tag, 3)}};
    ResultWait w(spy_sync, &spy, kShort, kLong);
    CHECK(w.own_word(b.get(), tag) == kWordsOk && spy.calls == 1 && w.synced() && word::value(b.get()) == 3);
  }
  {  // the stream wait fails
    Spy spy;
    spy.ok = false;
    Block b = block(2, 0);
    ResultWait w(spy_sync, &spy, kShort, kLong);
    CHECK(w.own_word(b.get(), tag) == kWordsSyncFailed && spy.calls == 1 && !w.synced());
    CHECK(w.own_word(b.get() + 1, tag) == kWordsSyncFailed && spy.calls == 1);
  }
  {  // lenient: the caller decodes and reports
    Spy spy;
    Block b = block(1, 0);
    ResultWait w(spy_sync, &spy, kShort, kLong);
    CHECK(w.own([&] { return word::ready(b.get(), tag); }, true) == kWordsOk && spy.calls == 1 && w.synced());
  }
  for (uint32_t t : {1u, 0x1234u, 0x80000000u, 0x80000001u, 0xffffffffu}) {  // tags
    Block b = block(1, 0);
    for (uint32_t other : {t - 1, 0u, t ^ 0x80000000u, t + 1}) {
      if (other == t) continue;
      b[0] = word::make(other, 1);
      CHECK(!word::ready(b.get(), t));
      Spy spy;
      ResultWait w(spy_sync, &spy, kShort, kLong);
      CHECK(w.own_word(b.get(), t) == kWordsNotWritten);
    }
    b[0] = word::make(t, 0xfffffffeu);
    CHECK(word::ready(b.get(), t) && word::value(b.get()) == 0xfffffffeu && word::ivalue(b.get()) == -2);
    CHECK(b[0] == (static_cast<uint64_t>(t) << 32 | 0xfffffffeu));
  }
  {  // a peer past its limit: the rank is named, the stream is left alone
    Spy spy;
    Block b = block(1, word::make(tag - 1, 1));
    ResultWait w(spy_sync, &spy, kLong, kShort);
    CHECK(w.peer_word(b.get(), tag, 7) == kWordsPeerSilent && w.silent_rank() == 7 && spy.calls == 0 && !w.synced());
    b[0] = word::make(tag, 1);
    CHECK(w.peer_word(b.get(), tag, 7) == kWordsOk);
  }
  return true;
}

// ---- random candidate lists
struct Case {
  std::vector<int32_t> cand_src, cand_off{0}, status_host, drain, mapv;
  int32_t max_np = 0;
  int32_t n_input() const { return static_cast<int32_t>(status_host.size()); }
  int32_t n_cand() const { return static_cast<int32_t>(cand_src.size()); }
  CandView view() const {
    return CandView{cand_src.data(), cand_off.data(), status_host.data(), n_cand(), n_input(), max_np};
  }
  std::vector<int32_t> map_of(int32_t k) const { return {mapv.begin() + cand_off[k], mapv.begin() + cand_off[k + 1]}; }
};

Case gen_case(int n_max, int p_drain_of_6) {
  Case c;
  const int n = pick(0, n_max);
  for (int i = 0; i < n; ++i) {
    const int kind = pick(0, 9);
    c.status_host.push_back(kind == 0 ? kFallback : kind <= 2 ? kEmpty : kPending);
    if (kind <= 2) continue;
    const int np = pick(0, 4);
    c.cand_src.push_back(i);
    c.cand_off.push_back(c.cand_off.back() + np);
    c.drain.push_back(pick(1, 6) <= p_drain_of_6);
    for (int q = 0; q < np; ++q) c.mapv.push_back(pick(0, 3) ? pick(0, 5000) : 0x7fffffff);
    c.max_np = std::max(c.max_np, np);
  }
  return c;
}

struct Corners {
  // early
  long e_none = 0, e_first = 0, e_last = 0, e_nowin = 0, e_zero = 0, e_reverse = 0, e_unwritten = 0;
  // sequence
  long s_floor_m1 = 0, s_floor_mid = 0, s_floor_last = 0, s_stale_below = 0, s_no_active = 0, s_fallback_stop = 0;
  long s_empty_at[3] = {0, 0, 0}, s_fallback_at[3] = {0, 0, 0};  // before / between / after the active ones above the floor
  long late_map = 0;  // mappings of two words or more delivered from the writer thread, status first
  // shared memory
  long m_own = 0, m_peer = 0, m_nowin = 0, m_ff = 0, m_noff = 0, m_nx = 0, m_nonx = 0, m_norank = 0, m_gaps = 0,
       m_codes = 0, m_uneven = 0;
} g_seen;

// ---- the early walk
bool check_early(const Case& c, uint32_t tag, int order) {
  const int32_t n = c.n_cand(), pods = c.cand_off.back();
  int32_t W = -1;  // naive: every value at once
  for (int32_t k = n - 1; k >= 0; --k)
    if (c.drain[k]) W = k;
  Block stat = block(static_cast<size_t>(n), 0), map = block(static_cast<size_t>(pods), 0);
  for (int32_t k = 0; k < n; ++k) stat[k] = stale(tag, 1);
  for (int32_t q = 0; q < pods; ++q) map[q] = stale(tag, 7777);
  std::vector<Store> s;
  // (the candidates after the winner are never written)
  for (int32_t k = 0; k <= (W >= 0 ? W : n - 1); ++k) s.push_back({stat.get() + k, word::make(tag, c.drain[k])});
  const std::vector<int32_t> want = W >= 0 ? c.map_of(W) : std::vector<int32_t>();
  if (W >= 0) map_stores(&s, map.get() + c.cand_off[W], want, tag);
  Spy spy;
  ResultWait w(spy_sync, &spy, kLong, kLong);
  Walk r;
  Seen got;
  {
    auto dev = deliver(s, order);
    r = walk_early(stat.get(), map.get(), c.view(), tag, w);
    got = see(r.map, r.np, tag, want.size());
  }
  CHECK(r.st == kWordsOk && spy.calls == 0 && !w.synced());
  CHECK(r.winner == W);
  CHECK(got.is(want));
  g_seen.late_map += order == 1 && want.size() >= 2;
  g_seen.e_none += n == 0;
  g_seen.e_first += W == 0;
  g_seen.e_last += n > 1 && W == n - 1;
  g_seen.e_nowin += n > 0 && W < 0;
  g_seen.e_zero += W >= 0 && r.np == 0;
  g_seen.e_reverse += order == 2 && s.size() > 2;
  g_seen.e_unwritten += W >= 0 && W < n - 1;
  return true;
}

// ---- the sequence walk
bool check_sequence(const Case& c, uint32_t tag, int32_t floor, int order) {
  const int32_t n = c.n_input(), na = c.n_cand(), pods = c.cand_off.back();
  // naive: the first drainable active candidate and the first fallback candidate above the floor, whichever is
  // first decides
  int32_t W = INT32_MAX, Wk = -1, F = INT32_MAX;
  for (int32_t k = na - 1; k >= 0; --k)
    if (c.cand_src[k] > floor && c.drain[k]) W = c.cand_src[k], Wk = k;
  for (int32_t i = n - 1; i > floor; --i)
    if (c.status_host[i] == kFallback) F = i;
  CHECK(first_fallback_above(c.view(), floor) == F);
  const int32_t winner = W < F ? W : -1, fallback = W < F ? -1 : F == INT32_MAX ? -1 : F;
  const int32_t end = winner >= 0 ? winner : fallback >= 0 ? fallback - 1 : n - 1;
  Block stat = block(static_cast<size_t>(na), 0), map = block(static_cast<size_t>(pods), 0);
  for (int32_t k = 0; k < na; ++k) stat[k] = stale(tag, 1);
  for (int32_t q = 0; q < pods; ++q) map[q] = stale(tag, 7777);
  std::vector<Store> s;
  bool below = false, any_above = false;
  for (int32_t k = 0; k < na; ++k) {
    const int32_t i = c.cand_src[k];
    below |= i <= floor;
    any_above |= i > floor;
    if (i > floor && i <= end) s.push_back({stat.get() + k, word::make(tag, c.drain[k])});
  }
  const std::vector<int32_t> want = winner >= 0 ? c.map_of(Wk) : std::vector<int32_t>();
  if (winner >= 0) map_stores(&s, map.get() + c.cand_off[Wk], want, tag);
  Spy spy;
  ResultWait w(spy_sync, &spy, kLong, kLong);
  Walk r;
  Seen got;
  {
    auto dev = deliver(s, order);
    r = walk_sequence(stat.get(), map.get(), c.view(), tag, floor, w);
    got = see(r.map, r.np, tag, want.size());
  }
  CHECK(r.st == kWordsOk && spy.calls == 0);
  CHECK(r.winner == winner && r.fallback == fallback && r.end == end);
  CHECK(got.is(want));
  g_seen.late_map += order == 1 && want.size() >= 2;
  // where the host-decided candidates the walk passed (empty) or stopped at (fallback) lie among the active
  // candidates above the floor
  int32_t first_act = -1, last_act = -1;
  for (int32_t k = 0; k < na; ++k)
    if (c.cand_src[k] > floor) {
      if (first_act < 0) first_act = c.cand_src[k];
      last_act = c.cand_src[k];
    }
  for (int32_t i = floor + 1; i <= std::min(n - 1, fallback >= 0 ? fallback : end); ++i) {
    if (c.status_host[i] == kPending || first_act < 0) continue;
    const int at = i < first_act ? 0 : i < last_act ? 1 : 2;
    (c.status_host[i] == kFallback ? g_seen.s_fallback_at : g_seen.s_empty_at)[at] += 1;
  }
  g_seen.s_floor_m1 += floor == -1 && n > 0;
  g_seen.s_floor_mid += floor > 0 && floor < n - 1;
  g_seen.s_floor_last += n > 0 && floor == n - 1;
  g_seen.s_stale_below += below && any_above;
  g_seen.s_no_active += n > 0 && !any_above && floor < n - 1;
  g_seen.s_fallback_stop += fallback >= 0;
  return true;
}

// ---- the ledger round
bool check_ledger_one(int n_header, int32_t n, int32_t max_np, int32_t floor, int32_t stop, int32_t win, int32_t np,
                      int order, WordsStatus want) {
  const uint32_t tag = 0x80000000u + static_cast<uint32_t>(pick(1, 1 << 20));
  const bool valid = win >= 0 && want == kWordsOk;
  // (an invalid winner's mapping does not exist: the walk must not look for it)
  const int32_t n_map = valid ? np : 0;
  Block words = block(static_cast<size_t>(n_header + n_map), 0);
  for (int32_t i = 0; i < n_header + n_map; ++i) words[i] = stale(tag, 3);
  std::vector<int32_t> mapv;
  std::vector<Store> s = {{words.get(), word::make(tag, static_cast<uint32_t>(win))},
                          {words.get() + 1, word::make(tag, static_cast<uint32_t>(np))}};
  for (int i = 2; i < n_header; ++i) s.push_back({words.get() + i, word::make(tag, 0)});
  for (int32_t q = 0; q < n_map; ++q) mapv.push_back(pick(0, 5000));
  map_stores(&s, words.get() + n_header, mapv, tag);
  const CandView v{nullptr, nullptr, nullptr, 0, n, max_np};
  Spy spy;
  ResultWait w(spy_sync, &spy, kLong, kLong);
  Walk r;
  Seen got;
  {
    auto dev = deliver(s, order % 4);
    r = walk_ledger(words.get(), n_header, v, tag, floor, stop, w);
    if (r.st == kWordsOk) got = see(r.map, r.np, tag, mapv.size());
  }
  CHECK(r.st == want && spy.calls == 0);
  if (want != kWordsOk) return true;
  if (win >= 0) {
    CHECK(r.winner == win && r.end == win && r.fallback == -1 && got.is(mapv));
  } else if (stop != INT32_MAX) {
    CHECK(r.winner == -1 && r.fallback == stop && r.end == stop - 1);
  } else {
    CHECK(r.winner == -1 && r.fallback == -1 && r.end == n - 1);
  }
  return true;
}

bool check_ledger() {
  const int32_t n = 9, max_np = 4, floor = 3;
  for (int order = 0; order < 8; ++order) {
    const int n_header = order < 4 ? 2 : 3;
    bool ok = check_ledger_one(n_header, n, max_np, floor, 6, -1, 0, order, kWordsOk) &&           // no winner, a stop
              check_ledger_one(n_header, n, max_np, floor, INT32_MAX, -1, 0, order, kWordsOk) &&   // no winner, no stop
              check_ledger_one(n_header, n, max_np, floor, INT32_MAX, floor + 1, 2, order, kWordsOk) &&
              check_ledger_one(n_header, n, max_np, floor, 8, n - 1, max_np, order, kWordsOk) &&
              check_ledger_one(n_header, n, max_np, floor, 8, 5, 0, order, kWordsOk) &&  // (a winner without pods)
              check_ledger_one(n_header, n, max_np, -1, INT32_MAX, 0, 1, order, kWordsOk) &&
              check_ledger_one(n_header, n, max_np, floor, 6, floor, 1, order, kWordsNoCandidate) &&
              check_ledger_one(n_header, n, max_np, floor, 6, 0, 1, order, kWordsNoCandidate) &&
              check_ledger_one(n_header, n, max_np, floor, 6, n, 1, order, kWordsNoCandidate) &&
              check_ledger_one(n_header, n, max_np, floor, 6, 5, -1, order, kWordsNoCandidate) &&
              check_ledger_one(n_header, n, max_np, floor, 6, 5, max_np + 1, order, kWordsNoCandidate) &&
              check_ledger_one(n_header, n, max_np, floor, 6, 5, INT32_MAX, order, kWordsNoCandidate);
    if (!ok) return false;
  }
  // a header word that never comes
  const int n_header = 2;
  Block words = block(n_header, 0);
  words[0] = word::make(5, static_cast<uint32_t>(-1));
  Spy spy;
  ResultWait w(spy_sync, &spy, kShort, kLong);
  const CandView v{nullptr, nullptr, nullptr, 0, n, max_np};
  CHECK(walk_ledger(words.get(), n_header, v, 5, floor, 6, w).st == kWordsNotWritten && spy.calls == 1);
  return true;
}

// ---- K3's header
bool check_header() {
  for (int n_header : {8, 5, 11})
  for (int order = 0; order < 4; ++order)
    for (int owner = 0; owner < 2; ++owner) {
      const uint32_t tag = static_cast<uint32_t>(pick(1, 1 << 30));
      const int32_t np = order == 1 ? pick(2, 5) : pick(0, 5), first_ok = owner ? pick(0, 90) : pick(-1, 90);
      const int32_t ff = pick(-1, 90), nx = pick(-1, 90);
      // owner flag 0: there is no mapping behind the header, whatever the pod count says
      const int32_t n_map = owner ? np : 0;
      Block res = block(static_cast<size_t>(n_header + n_map), 0);
      for (int32_t i = 0; i < n_header + n_map; ++i) res[i] = stale(tag, 1);
      std::vector<int32_t> mapv;
      std::vector<Store> s = {{res.get() + kResFirstOk, word::make(tag, static_cast<uint32_t>(first_ok))},
                              {res.get() + kResOwner, word::make(tag, static_cast<uint32_t>(owner))},
                              {res.get() + kResPods, word::make(tag, owner ? static_cast<uint32_t>(np) : 5u)},
                              {res.get() + kResFirstFallback, word::make(tag, static_cast<uint32_t>(ff))},
                              {res.get() + kResRankNext, word::make(tag, static_cast<uint32_t>(nx))}};
      for (int32_t q = 0; q < n_map; ++q) mapv.push_back(pick(0, 5000));
      map_stores(&s, res.get() + n_header, mapv, tag);
      Spy spy;
      ResultWait w(spy_sync, &spy, kLong, kLong);
      WordsStatus st;
      Header h;
      Seen got;
      {
        auto dev = deliver(s, order);
        st = poll_header(res.get(), n_header, tag, w);
        h = read_header(res.get(), n_header, tag);
        got = see(h.map, h.np, tag, mapv.size());
      }
      CHECK(st == kWordsOk && spy.calls == 0);
      CHECK(h.st == kWordsOk && h.first_ok == first_ok && h.first_fallback == ff && h.rank_next == nx);
      CHECK(got.is(mapv));
    }
  const int n_header = 8;
  // a stale header: the poll falls back to the stream once and leaves the verdict to the decoding
  for (int field = 0; field < kResFields; ++field) {
    const uint32_t tag = 77;
    Block res = block(n_header, 0);
    for (int i = 0; i < kResFields; ++i) res[i] = word::make(i == field ? tag - 1 : tag, 0);
    Spy spy;
    ResultWait w(spy_sync, &spy, kShort, kLong);
    CHECK(poll_header(res.get(), n_header, tag, w) == kWordsOk && spy.calls == 1 && w.synced());
    CHECK(read_header(res.get(), n_header, tag).st == kWordsNotWritten);
    spy.ok = false;
    ResultWait w2(spy_sync, &spy, kShort, kLong);
    CHECK(poll_header(res.get(), n_header, tag, w2) == kWordsSyncFailed);
  }
  return true;
}

// ---- the shared-memory transport: N ranks as threads on one block
struct RankTick {
  Case c;
  int32_t base = 0, first_fallback = -1;
  uint64_t rank_next = ~0ull;
};
struct Expect {
  int64_t first_ok = -1, ff = -1, nx = -1;
  int32_t owner = -1, owner_k = -1;
};

// naive: every rank's candidates flattened, sorted by global index; the first drainable one
Expect naive_merge(const std::vector<RankTick>& ranks) {
  const int32_t N = static_cast<int32_t>(ranks.size());
  struct Flat {
    int64_t g;
    int32_t r, k;
  };
  std::vector<Flat> flat;
  Expect e;
  for (int32_t r = 0; r < N; ++r) {
    const RankTick& t = ranks[r];
    for (int32_t k = 0; k < t.c.n_cand(); ++k)
      if (t.c.drain[k]) flat.push_back({(static_cast<int64_t>(t.base) + t.c.cand_src[k]) * N + r, r, k});
    if (t.first_fallback >= 0) e.ff = e.ff < 0 ? t.first_fallback : std::min<int64_t>(e.ff, t.first_fallback);
    if (t.rank_next != ~0ull)
      e.nx = e.nx < 0 ? static_cast<int64_t>(t.rank_next) : std::min(e.nx, static_cast<int64_t>(t.rank_next));
  }
  std::sort(flat.begin(), flat.end(), [](const Flat& a, const Flat& b) { return a.g < b.g; });
  if (!flat.empty()) e.first_ok = flat[0].g, e.owner = flat[0].r, e.owner_k = flat[0].k;
  return e;
}

bool shm_rank(const ShmSeg& seg, const std::vector<std::vector<RankTick>>& plan, const std::vector<Expect>& expect,
              uint32_t seed) {
  std::mt19937 rng(seed);
  const int32_t r = seg.rank;
  for (uint64_t tick = 1; tick <= plan.size(); ++tick) {
    const RankTick& t = plan[tick - 1][r];
    const Expect& e = expect[tick - 1];
    const Case& c = t.c;
    Spy spy;
    ResultWait gate(spy_sync, &spy, kLong, kLong);
    const ShmPublished pub = shm_publish(seg, tick, c.view(), t.base, t.first_fallback, t.rank_next, gate);
    CHECK(pub.st == kWordsOk && pub.p == static_cast<int>(tick & 1) && pub.tag == shm_tag(seg.session, tick));
    const volatile uint64_t* reg = shm_region(seg, r, pub.p);
    CHECK(pub.stat == shm_region(seg, r, pub.p) + kShmHdr + seg.max_cand);
    CHECK(word::load(reg + kShmCount) == word::make(pub.tag, static_cast<uint32_t>(c.n_input())));
    CHECK(word::load(reg + kShmBase) == word::make(pub.tag, c.n_input() ? static_cast<uint32_t>(t.base + 1) : 0u));
    for (int32_t i = 0, k = 0; i < c.n_input(); ++i) {
      const bool active = c.status_host[i] == kPending;
      const uint32_t want = active ? static_cast<uint32_t>(k++) << 2 : c.status_host[i] == kFallback ? kInFallback : kInNoPods;
      CHECK(word::load(reg + kShmHdr + i) == word::make(pub.tag, want));
    }
    const int32_t pods = c.cand_off.back();
    Block own_map = block(static_cast<size_t>(pods), 0), res = block(static_cast<size_t>(kHeader + c.max_np), 0);
    for (int32_t q = 0; q < pods; ++q) own_map[q] = word::make(pub.tag - 1, 7777);
    for (int32_t q = 0; q < kHeader + c.max_np; ++q) res[q] = word::make(pub.tag - 1, 1);
    // this rank's K2: its outcome words (those after the tick's winner perhaps never), the drainable
    // candidates' mappings
    std::vector<Store> s;
    const bool lazy = rng() & 1;
    for (int32_t k = 0; k < c.n_cand(); ++k) {
      const int64_t g = (static_cast<int64_t>(t.base) + c.cand_src[k]) * seg.nranks + r;
      if (lazy && e.first_ok >= 0 && g > e.first_ok) continue;
      s.push_back({pub.stat + k, word::make(pub.tag, c.drain[k])});
      if (c.drain[k])
        for (int32_t q = c.cand_off[k]; q < c.cand_off[k + 1]; ++q)
          s.push_back({own_map.get() + q, word::make(pub.tag, static_cast<uint32_t>(c.mapv[q]))});
    }
    std::shuffle(s.begin(), s.end(), rng);
    ResultWait w(spy_sync, &spy, kLong, kLong);
    WordsStatus st;
    {
      Writer dev(std::move(s), rng() % 3 ? 0 : 100);
      st = shm_reduce(seg, pub.p, pub.tag, c.view(), own_map.get(), res.get(), kHeader, w);
    }
    CHECK(st == kWordsOk && spy.calls == 0);
    CHECK(word::load(reg + kShmDone) == word::make(pub.tag, 1));
    const Header h = read_header(res.get(), kHeader, pub.tag);
    CHECK(h.st == kWordsOk);
    CHECK(h.first_ok == static_cast<int32_t>(e.first_ok) && h.first_fallback == static_cast<int32_t>(e.ff) &&
          h.rank_next == static_cast<int32_t>(e.nx));
    CHECK(word::value(res.get() + kResOwner) == (e.owner == r ? 1u : 0u));
    if (e.owner == r) {
      CHECK(see(h.map, h.np, pub.tag, c.map_of(e.owner_k).size()).is(c.map_of(e.owner_k)));
      CHECK(word::ivalue(res.get() + kResPods) == h.np);
    } else {
      CHECK(h.np == 0 && word::value(res.get() + kResPods) == 0);
    }
  }
  return true;
}

bool check_shm_run(int32_t N, int ticks, int32_t max_cand) {
  const uint32_t session = g_rng();
  std::vector<std::vector<RankTick>> plan(static_cast<size_t>(ticks));
  std::vector<Expect> expect;
  for (auto& ranks : plan) {
    ranks.resize(static_cast<size_t>(N));
    const int32_t common = pick(0, 3);
    bool gaps = false, uneven = false, codes = false;
    for (int32_t r = 0; r < N; ++r) {
      RankTick& t = ranks[r];
      t.c = gen_case(pick(0, 4) ? max_cand : 0, pick(0, 4));
      t.base = pick(0, 2) ? common : pick(0, 4);
      const int32_t n = t.c.n_input();
      for (int32_t i = n - 1; i >= 0; --i)
        if (t.c.status_host[i] == kFallback) t.first_fallback = (t.base + i) * N + r, codes = true;
      if (pick(0, 1)) t.rank_next = static_cast<uint64_t>((t.base + n) * N + r);
      gaps |= n > 0 && ranks[0].c.n_input() > 0 && t.base != ranks[0].base;
      uneven |= n != ranks[0].c.n_input();
      g_seen.m_norank += n == 0;
    }
    const Expect e = naive_merge(ranks);
    expect.push_back(e);
    g_seen.m_own += e.owner == 0;
    g_seen.m_peer += e.owner > 0;
    g_seen.m_nowin += e.owner < 0;
    (e.ff >= 0 ? g_seen.m_ff : g_seen.m_noff) += 1;
    (e.nx >= 0 ? g_seen.m_nx : g_seen.m_nonx) += 1;
    g_seen.m_gaps += gaps;
    g_seen.m_uneven += uneven;
    g_seen.m_codes += codes;
  }
  const size_t words = static_cast<size_t>(N) * 2 * shm_region_words(max_cand);
  Block seg_words = block(words, 0);  // (a fresh segment holds zeros)
  std::vector<std::thread> threads;
  std::atomic<bool> ok{true};
  for (int32_t r = 0; r < N; ++r) {
    const uint32_t seed = g_rng();
    threads.emplace_back([&, r, seed] {
      const ShmSeg seg{seg_words.get(), max_cand, N, r, session};
      if (!shm_rank(seg, plan, expect, seed)) ok = false;
    });
  }
  for (auto& t : threads) t.join();
  return ok;
}

// The publish gate and the silent peer, step by step on two ranks.
bool check_shm_gate() {
  const int32_t N = 2, max_cand = 2;
  const uint32_t session = 0x7ffffff0u;  // (session + tick wraps into the tag's high bit)
  Block seg_words = block(static_cast<size_t>(N) * 2 * shm_region_words(max_cand), 0);
  const ShmSeg seg{seg_words.get(), max_cand, N, 0, session};
  Case c = gen_case(0, 0);
  Spy spy;
  // ticks 1 and 2: no gate (nobody has used the regions)
  for (uint64_t tick : {1, 2}) {
    ResultWait w(spy_sync, &spy, kLong, kShort);
    CHECK(shm_publish(seg, tick, c.view(), 0, -1, ~0ull, w).st == kWordsOk);
  }
  // tick 3 waits for both ranks' done words of tick 1 ...
  volatile uint64_t* done0 = shm_region(seg, 0, 1) + kShmDone;
  volatile uint64_t* done1 = shm_region(seg, 1, 1) + kShmDone;
  {
    ResultWait w(spy_sync, &spy, kLong, kShort);
    CHECK(shm_publish(seg, 3, c.view(), 0, -1, ~0ull, w).st == kWordsPeerSilent && w.silent_rank() == 0);
  }
  *done0 = word::make(shm_tag(session, 1), 1);
  *done1 = word::make(shm_tag(session, 1), 0);  // (the tag alone does not open the gate)
  {
    ResultWait w(spy_sync, &spy, kLong, kShort);
    CHECK(shm_publish(seg, 3, c.view(), 0, -1, ~0ull, w).st == kWordsPeerSilent && w.silent_rank() == 1);
  }
  // ... and proceeds when the last rank writes its word
  {
    std::atomic<bool> started{false};
    ResultWait w(spy_sync, &spy, kLong, kLong);
    ShmPublished pub;
    {
      Writer peer({{done1, word::make(shm_tag(session, 1), 1)}}, 2000, &started);
      pub = shm_publish(seg, 3, c.view(), 0, -1, ~0ull, w);
      CHECK(started.load());
    }
    CHECK(pub.st == kWordsOk && pub.p == 1 && pub.tag == shm_tag(session, 3) && (pub.tag & 0x80000000u));
  }
  // the walk of tick 3: rank 1 has published nothing for it
  {
    Block res = block(kHeader, 0);
    ResultWait w(spy_sync, &spy, kLong, kShort);
    CHECK(shm_reduce(seg, 1, shm_tag(session, 3), c.view(), nullptr, res.get(), kHeader, w) == kWordsPeerSilent);
    CHECK(w.silent_rank() == 1 && spy.calls == 0);
    CHECK(!word::ready(res.get(), shm_tag(session, 3)));
  }
  // this rank's own outcome word missing: the stream, once, then the error
  {
    Case one;
    one.status_host = {kPending};
    one.cand_src = {0};
    one.cand_off = {0, 1};
    one.drain = {1};
    one.mapv = {4};
    one.max_np = 1;
    Block words1 = block(2 * shm_region_words(max_cand), 0), res = block(kHeader + 1, 0), own_map = block(1, 0);
    const ShmSeg solo{words1.get(), max_cand, 1, 0, session};
    ResultWait w(spy_sync, &spy, kShort, kLong);
    const ShmPublished pub = shm_publish(solo, 1, one.view(), 0, -1, ~0ull, w);
    CHECK(pub.st == kWordsOk);
    CHECK(shm_reduce(solo, pub.p, pub.tag, one.view(), own_map.get(), res.get(), kHeader, w) == kWordsNotWritten);
    CHECK(spy.calls == 1 && w.synced());
  }
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  const int cases = argc > 1 ? std::atoi(argv[1]) : 1500;
  const uint32_t seed = argc > 2 ? static_cast<uint32_t>(std::strtoul(argv[2], nullptr, 10)) : 1u;
  g_rng.seed(seed);
  bool ok = check_wait() && check_ledger() && check_header() && check_shm_gate();
  for (int i = 0; ok && i < cases; ++i) {
    const uint32_t tag = pick(0, 9) == 0 ? 0xffffffffu : pick(0, 1) ? g_rng() | 0x80000000u : (g_rng() & 0x7fffffffu) | 1u;
    const Case c = gen_case(12, i % 7 == 0 ? 0 : pick(1, 3));
    const int n = c.n_input();
    ok = check_early(c, tag, i % 4);
    const int32_t floor = n == 0 ? -1 : i % 3 == 0 ? -1 : i % 3 == 1 ? n - 1 : pick(-1, n - 1);
    ok = ok && check_sequence(c, tag, floor, (i / 4) % 4);
  }
  const int runs = std::max(1, cases / 50);
  for (int i = 0; ok && i < runs; ++i) ok = check_shm_run(1 + i % 3, pick(5, 12), pick(1, 6));
  if (!ok || g_failures) {
    std::fprintf(stderr, "result_words_check: FAILED (seed %u)\n", seed);
    return 1;
  }
  const Corners& s = g_seen;
  const bool early = s.e_none && s.e_first && s.e_last && s.e_nowin && s.e_zero && s.e_reverse && s.e_unwritten;
  const bool seq = s.s_floor_m1 && s.s_floor_mid && s.s_floor_last && s.s_stale_below && s.s_empty_at[0] &&
                   s.s_empty_at[1] && s.s_empty_at[2] && s.s_fallback_at[0] && s.s_fallback_at[1] && s.s_fallback_at[2] &&
                   s.s_no_active && s.s_fallback_stop && s.late_map;
  const bool shm = s.m_own && s.m_peer && s.m_nowin && s.m_ff && s.m_noff && s.m_nx && s.m_nonx && s.m_norank &&
                   s.m_gaps && s.m_codes && s.m_uneven;
  if (!(early && seq && shm)) {
    std::fprintf(stderr, "result_words_check: a vacuous run (early %d, sequence %d, shared memory %d; seed %u)\n", early,
                 seq, shm, seed);
    return 2;
  }
  std::printf("result_words_check ok: %d lists (early: %ld no winner, %ld zero-pod winners, %ld with unwritten words; "
              "sequence: %ld fallback stops, %ld with stale words below the floor), %d shared-memory runs (%ld ticks "
              "won here, %ld by a peer, %ld by nobody, %ld with gaps)\n",
              cases, s.e_nowin, s.e_zero, s.e_unwritten, s.s_fallback_stop, s.s_stale_below, runs, s.m_own, s.m_peer,
              s.m_nowin, s.m_gaps);
  return 0;
}
