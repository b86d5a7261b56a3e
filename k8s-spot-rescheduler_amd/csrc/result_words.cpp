// result_words.cpp — the host walks over the tagged result words (result_words.hpp).
#include "result_words.hpp"

#include <algorithm>
#include <climits>
#include <vector>

#include "../../include/sr_planner.h"

namespace sr {

int32_t first_fallback_above(const CandView& c, int32_t floor) {
  for (int32_t i = floor + 1; i < c.n_input_cand; ++i)
    if (c.status_host[i] == SR_CAND_FALLBACK) return i;
  return INT32_MAX;
}

namespace {

// The mapping of active candidate k, waited for.
void take_map(Walk* r, int32_t k, const volatile uint64_t* map, const CandView& c, uint32_t tag, ResultWait& wait) {
  r->map = map + c.cand_off[k];
  r->np = c.cand_off[k + 1] - c.cand_off[k];
  r->st = wait.own_span(r->map, r->np, tag);
}

}  // namespace

Walk walk_early(const volatile uint64_t* stat, const volatile uint64_t* map, const CandView& c, uint32_t tag,
                ResultWait& wait) {
  Walk r;
  for (int32_t k = 0; k < c.n_cand; ++k) {
    if ((r.st = wait.own_word(stat + k, tag)) != kWordsOk) return r;
    if (word::value(stat + k) == 1) {
      r.winner = k;
      take_map(&r, k, map, c, tag, wait);
      break;
    }
  }
  return r;
}

Walk walk_sequence(const volatile uint64_t* stat, const volatile uint64_t* map, const CandView& c, uint32_t tag,
                   int32_t floor, ResultWait& wait) {
  Walk r;
  r.end = c.n_input_cand - 1;
  // the active candidates ascend in the caller's index (cand_src): k follows i
  int32_t k = static_cast<int32_t>(std::upper_bound(c.cand_src, c.cand_src + c.n_cand, floor) - c.cand_src);
  for (int32_t i = floor + 1; i < c.n_input_cand; ++i) {
    if (k < c.n_cand && c.cand_src[k] == i) {
      if ((r.st = wait.own_word(stat + k, tag)) != kWordsOk) return r;
      if (word::value(stat + k) == 1) {
        r.winner = r.end = i;
        take_map(&r, k, map, c, tag, wait);
        break;
      }
      ++k;
    } else if (c.status_host[i] == SR_CAND_FALLBACK) {
      r.fallback = i;
      r.end = i - 1;
      break;
    }
  }
  return r;
}

Walk walk_ledger(const volatile uint64_t* words, int32_t n_header, const CandView& c, uint32_t tag, int32_t floor,
                 int32_t stop, ResultWait& wait) {
  Walk r;
  r.end = c.n_input_cand - 1;
  for (int32_t i = 0; i < n_header; ++i)
    if ((r.st = wait.own_word(words + i, tag)) != kWordsOk) return r;
  const int32_t win = word::ivalue(words), np = word::ivalue(words + 1);
  if (win >= 0) {
    if (win <= floor || win >= c.n_input_cand || np < 0 || np > c.max_cand_pods) {
      r.st = kWordsNoCandidate;
      return r;
    }
    r.map = words + n_header;
    r.np = np;
    if ((r.st = wait.own_span(r.map, np, tag)) != kWordsOk) return r;
    r.winner = r.end = win;
  } else if (stop != INT32_MAX) {
    r.fallback = stop;
    r.end = stop - 1;
  }
  return r;
}

WordsStatus poll_header(const volatile uint64_t* res, int32_t n_header, uint32_t tag, ResultWait& wait) {
  auto all_ready = [=] {
    for (int32_t i = 0; i < kResFields; ++i)
      if (!word::ready(res + i, tag)) return false;
    if (!word::value(res + kResOwner)) return true;
    const volatile uint64_t* map = res + n_header;
    for (uint32_t q = 0, np = word::value(res + kResPods); q < np; ++q)
      if (!word::ready(map + q, tag)) return false;
    return true;
  };
  const WordsStatus st = wait.own(all_ready, true);
  std::atomic_thread_fence(std::memory_order_acquire);
  return st;
}

Header read_header(const volatile uint64_t* res, int32_t n_header, uint32_t tag) {
  Header h;
  for (int32_t i = 0; i < kResFields; ++i)
    if (!word::ready(res + i, tag)) {
      h.st = kWordsNotWritten;
      return h;
    }
  h.first_ok = word::ivalue(res + kResFirstOk);
  h.first_fallback = word::ivalue(res + kResFirstFallback);
  h.rank_next = word::ivalue(res + kResRankNext);
  if (word::value(res + kResOwner)) {
    h.np = word::ivalue(res + kResPods);
    h.map = res + n_header;
  }
  return h;
}

ShmPublished shm_publish(const ShmSeg& s, uint64_t tick, const CandView& c, int32_t base, int32_t first_fallback,
                         uint64_t rank_next, ResultWait& wait) {
  ShmPublished r;
  r.p = static_cast<int>(tick & 1);
  if (tick > 2) {
    const uint64_t done = word::make(shm_tag(s.session, tick - 2), 1);
    for (int32_t q = 0; q < s.nranks; ++q) {
      const volatile uint64_t* hd = shm_region(s, q, r.p) + kShmDone;
      if ((r.st = wait.peer([=] { return word::load(hd) == done; }, q)) != kWordsOk) return r;
    }
  }
  r.tag = shm_tag(s.session, tick);
  volatile uint64_t* reg = shm_region(s, s.rank, r.p);
  const int32_t n_in = c.n_input_cand;
  for (int32_t i = 0, k = 0; i < n_in; ++i) {  // (cand_src ascends: k follows i)
    const bool active = k < c.n_cand && c.cand_src[k] == i;
    reg[kShmHdr + i] = word::make(r.tag, active ? static_cast<uint32_t>(k++ << 2)
                                         : c.status_host[i] == SR_CAND_FALLBACK ? kInFallback : kInNoPods);
  }
  std::atomic_thread_fence(std::memory_order_release);
  reg[kShmCount] = word::make(r.tag, static_cast<uint32_t>(n_in));
  reg[kShmBase] = word::make(r.tag, static_cast<uint32_t>(n_in > 0 ? base + 1 : 0));
  reg[kShmFirstFallback] = word::make(r.tag, static_cast<uint32_t>(first_fallback + 1));
  reg[kShmRankNext] = word::make(r.tag, static_cast<uint32_t>(rank_next == ~0ull ? 0 : rank_next + 1));
  r.stat = const_cast<uint64_t*>(reg) + kShmHdr + s.max_cand;
  return r;
}

WordsStatus shm_reduce(const ShmSeg& s, int p, uint32_t tag, const CandView& c, const volatile uint64_t* own_map,
                       volatile uint64_t* res, int32_t n_header, ResultWait& wait) {
  const int32_t N = s.nranks;
  auto smaller = [](int64_t a, int64_t b) { return b < 0 ? a : a < 0 ? b : std::min(a, b); };  // of those >= 0
  std::vector<int64_t> n_r(static_cast<size_t>(N)), b_r(static_cast<size_t>(N));
  int64_t ff = -1, nx = -1;
  for (int32_t r = 0; r < N; ++r) {
    const volatile uint64_t* hd = shm_region(s, r, p);
    for (int i : {kShmCount, kShmBase, kShmFirstFallback, kShmRankNext})
      if (WordsStatus st = wait.peer_word(hd + i, tag, r)) return st;
    std::atomic_thread_fence(std::memory_order_acquire);
    n_r[r] = word::value(hd + kShmCount);
    b_r[r] = static_cast<int64_t>(word::value(hd + kShmBase)) - 1;
    ff = smaller(ff, static_cast<int64_t>(word::value(hd + kShmFirstFallback)) - 1);
    nx = smaller(nx, static_cast<int64_t>(word::value(hd + kShmRankNext)) - 1);
  }
  int64_t first_ok = -1;
  int32_t owner = -1, oci = -1;
  std::vector<int64_t> at(static_cast<size_t>(N), 0);  // next input candidate of each rank
  for (;;) {
    int32_t r = -1;
    int64_t g = INT64_MAX;
    for (int32_t q = 0; q < N; ++q) {
      if (at[q] >= n_r[q]) continue;
      const int64_t gq = (b_r[q] + at[q]) * N + q;
      if (gq < g) g = gq, r = q;
    }
    if (r < 0) break;  // every planned index walked
    const volatile uint64_t* reg = shm_region(s, r, p);
    const volatile uint64_t* in = reg + kShmHdr + at[r]++;
    if (WordsStatus st = wait.peer_word(in, tag, r)) return st;
    const uint32_t v = word::value(in);
    if ((v & kInCodeMask) != kInActive) continue;  // no pods to move, or the reference path
    const int32_t ci = static_cast<int32_t>(v >> 2);
    const volatile uint64_t* sw = reg + kShmHdr + s.max_cand + ci;
    if (WordsStatus st = r == s.rank ? wait.own_word(sw, tag) : wait.peer_word(sw, tag, r)) return st;
    if (word::value(sw) & 1u) {
      first_ok = g;
      owner = r;
      oci = ci;
      break;
    }
  }
  shm_region(s, s.rank, p)[kShmDone] = word::make(tag, 1);  // this tick's words may be reused
  int32_t np = 0;
  if (owner == s.rank) {
    const int32_t off = c.cand_off[oci];
    np = c.cand_off[oci + 1] - off;
    for (int32_t q = 0; q < np; ++q) {
      if (WordsStatus st = wait.own_word(own_map + off + q, tag)) return st;
      res[n_header + q] = word::make(tag, word::value(own_map + off + q));
    }
  }
  res[kResFirstOk] = word::make(tag, static_cast<uint32_t>(first_ok));
  res[kResOwner] = word::make(tag, owner == s.rank ? 1u : 0u);
  res[kResPods] = word::make(tag, static_cast<uint32_t>(np));
  res[kResFirstFallback] = word::make(tag, static_cast<uint32_t>(ff));
  res[kResRankNext] = word::make(tag, static_cast<uint32_t>(nx));
  return kWordsOk;
}

}  // namespace sr
