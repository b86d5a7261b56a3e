// result_words.hpp — the tagged result words every run ends in, the one wait for them, and the host walks
// over them.
//
// HIP-free.  A run's outcome reaches the host as 64-bit words in mapped (or shared) memory, each
// tag << 32 | value, where tag is the run's sequence number: a word is this run's once its upper half equals
// the tag, whatever it held before.  The writers store them without ordering among each other (K2 per finished
// candidate, K3, the ledger step of sr_plan_sequence_pdb, another rank's host), so a reader polls exactly the
// words it needs, in the order it needs them, instead of waking up on stream completion.  planner.cpp owns the
// buffers, the stream, the launches and sr_ctx::in_flight; this unit owns the word, the wait and the walks.
// tools/result_words_check.cpp takes all of it through its corners on the host, a thread playing the device
// and the other ranks.
#pragma once

#include <atomic>
#include <chrono>
#include <cstddef>
#include <cstdint>

namespace sr {

// ---- the word.  The only volatile read of a result word is load().
namespace word {
inline uint64_t load(const volatile uint64_t* p) { return *p; }
inline bool ready(const volatile uint64_t* p, uint32_t tag) { return static_cast<uint32_t>(load(p) >> 32) == tag; }
inline uint32_t value(const volatile uint64_t* p) { return static_cast<uint32_t>(load(p)); }
inline int32_t ivalue(const volatile uint64_t* p) { return static_cast<int32_t>(value(p)); }
inline uint64_t make(uint32_t tag, uint32_t v) { return static_cast<uint64_t>(tag) << 32 | v; }
}  // namespace word

// The result header K3 writes into DevWorkload::result (and shm_reduce as K3 would); kernels.hpp's kResultHeader
// words lie before the winner's mapping.
enum ResultField {
  kResFirstOk = 0,        // first drainable candidate (global index, -1: none)
  kResOwner = 1,          // 1: this rank planned it (its mapping follows the header)
  kResPods = 2,           // pods of its mapping
  kResFirstFallback = 3,  // first fallback candidate (global index, -1: none)
  kResRankNext = 4,       // smallest global index no rank has planned yet (-1: none)
  kResFields = 5
};

// How a wait or a walk ended.  planner.cpp maps these to sr_status and its error texts.
enum WordsStatus {
  kWordsOk = 0,
  kWordsNotWritten,  // a word of this rank's own run is missing after the stream was waited for
  kWordsPeerSilent,  // another rank's word did not arrive within the peer limit (ResultWait::silent_rank)
  kWordsSyncFailed,  // the stream fallback itself failed (the callable recorded why)
  kWordsNoCandidate  // the ledger step's words name no candidate of the round
};

// ---- the wait: one per run.  Spins on a predicate; the clock is read every 1024th spin.
//   own word:  after own_limit the stream is waited for through `sync` (once per run; this also surfaces a
//              kernel fault as an error); a word still missing then was never written.
//   peer word: another rank's; after peer_limit (counted from this wait's first miss) that rank has stopped.
// A word that is there at entry costs its load alone.
class ResultWait {
 public:
  using clock = std::chrono::steady_clock;
  using SyncFn = bool (*)(void* user);  // waits for the run's stream; false: failed
  ResultWait(SyncFn sync, void* user, clock::duration own_limit = std::chrono::milliseconds(100),
             clock::duration peer_limit = std::chrono::seconds(60))
      : sync_(sync), user_(user), own_limit_(own_limit), peer_limit_(peer_limit) {}

  // lenient: a word still missing after the stream fallback is not an error here (the caller checks the tags
  // again when it decodes: read_header)
  template <class F>
  WordsStatus own(F ready, bool lenient = false) {
    if (ready()) return kWordsOk;
    if (sync_failed_) return kWordsSyncFailed;
    if (!synced_) {
      if (!started_) t0_ = clock::now(), started_ = true;
      if (!spin(ready, t0_, own_limit_)) (sync_(user_) ? synced_ : sync_failed_) = true;
      if (sync_failed_) return kWordsSyncFailed;
    }
    return lenient || ready() ? kWordsOk : kWordsNotWritten;
  }
  template <class F>
  WordsStatus peer(F ready, int32_t rank) {
    if (ready() || spin(ready, clock::now(), peer_limit_)) return kWordsOk;
    silent_rank_ = rank;
    return kWordsPeerSilent;
  }
  WordsStatus own_word(const volatile uint64_t* p, uint32_t tag) {
    return own([=] { return word::ready(p, tag); });
  }
  WordsStatus peer_word(const volatile uint64_t* p, uint32_t tag, int32_t rank) {
    return peer([=] { return word::ready(p, tag); }, rank);
  }
  // n consecutive own words, then the acquire fence their values are read behind
  WordsStatus own_span(const volatile uint64_t* p, int32_t n, uint32_t tag) {
    for (int32_t q = 0; q < n; ++q)
      if (WordsStatus st = own_word(p + q, tag)) return st;
    std::atomic_thread_fence(std::memory_order_acquire);
    return kWordsOk;
  }

  bool synced() const { return synced_; }  // a wait of this run waited for the stream: its device work is done
  int32_t silent_rank() const { return silent_rank_; }

 private:
  // The spin loop: until ready() (true), or until `limit` has passed since t0 (false).
  template <class F>
  bool spin(F ready, clock::time_point t0, clock::duration limit) {
    uint32_t spins = spins_;  // (a register while it spins)
    bool in_time = true;
    while (in_time && !ready()) in_time = (++spins & 1023) != 0 || clock::now() - t0 <= limit;
    spins_ = spins;
    return in_time;
  }

  SyncFn sync_;
  void* user_;
  clock::duration own_limit_, peer_limit_;
  clock::time_point t0_{};  // the run's first missing own word
  uint32_t spins_ = 0;
  int32_t silent_rank_ = -1;
  bool started_ = false, synced_ = false, sync_failed_ = false;
};

// ---- the walks.  What they read of a Workload (host.hpp), by the same names:
struct CandView {
  const int32_t* cand_src;     // [n_cand] the active candidates' indices in the caller's list, ascending
  const int32_t* cand_off;     // [n_cand + 1] their first active pod
  const int32_t* status_host;  // [n_input_cand] SR_CAND_EMPTY / SR_CAND_FALLBACK / pending
  int32_t n_cand, n_input_cand, max_cand_pods;
};

// The value halves of n ready words into dst.
inline void copy_values(const volatile uint64_t* words, int32_t n, int32_t* dst) {
  for (int32_t q = 0; q < n; ++q) dst[q] = word::ivalue(words + q);
}

// A walk's winner: the mapping words are ready and may be read (copy_values) when np > 0.
struct Walk {
  WordsStatus st = kWordsOk;
  int32_t winner = -1;    // early: the active candidate; a round: the caller's index (-1: none)
  int32_t fallback = -1;  // a round: the fallback candidate the walk stopped at
  int32_t end = -1;       // a round: the last candidate the walk judged
  int32_t np = 0;
  const volatile uint64_t* map = nullptr;
};

// The first fallback candidate above the floor (INT32_MAX: none).
int32_t first_fallback_above(const CandView& c, int32_t floor);

// The end of a single-rank winner-only run: K2's words `stat` [n_cand] seq << 32 | drainable in candidate order
// up to the first drainable candidate, then its mapping in `map` [active pods] (rescheduler.go:280-286 stops
// there too).  Words of later candidates are not touched.
Walk walk_early(const volatile uint64_t* stat, const volatile uint64_t* map, const CandView& c, uint32_t tag,
                ResultWait& wait);

// The end of a sequence round: as walk_early, but over the caller's candidates above the floor (the skipped
// candidates' waves store no word and may be scheduled last: the work list is in cost order), taking the
// host-decided ones in between (no pods: passed over; the reference path: the walk stops there).
Walk walk_sequence(const volatile uint64_t* stat, const volatile uint64_t* map, const CandView& c, uint32_t tag,
                   int32_t floor, ResultWait& wait);

// The end of a round under disruption budgets: the winner is the ledger step's (seq_pdb.hip), `words`
// {winner (-1: none), npods, mapping...} with n_header (kPdbHeader) words before the mapping.  stop: the round's
// first unrefused fallback candidate (INT32_MAX: none).  kWordsNoCandidate for a winner outside (floor,
// n_input_cand) or a pod count outside [0, max_cand_pods].
Walk walk_ledger(const volatile uint64_t* words, int32_t n_header, const CandView& c, uint32_t tag, int32_t floor,
                 int32_t stop, ResultWait& wait);

// K3's words: the header, then (owner flag set) the mapping of kResPods words behind n_header (kResultHeader)
// words.  poll_header waits for them, leniently; read_header decodes words that should be in place (after
// poll_header, a stream wait, or shm_reduce) and is the one to say kWordsNotWritten for a stale header.
struct Header {
  WordsStatus st = kWordsOk;
  int32_t first_ok = -1, first_fallback = -1, rank_next = -1;
  int32_t np = 0;  // 0 unless this rank owns the winner
  const volatile uint64_t* map = nullptr;
};
WordsStatus poll_header(const volatile uint64_t* res, int32_t n_header, uint32_t tag, ResultWait& wait);
Header read_header(const volatile uint64_t* res, int32_t n_header, uint32_t tag);

// ---- the shared-memory transport (sr_comm_init_shm): the ranks of one node reduce through host memory.  One
// segment holds, per rank r and tick parity p, a region of kShmHdr + 2 * max_cand words (tag: shm_tag of the
// tick, identical on every rank):
//   hdr    ShmField below
//   in[i]  input candidate i: active candidate << 2, or kInNoPods / kInFallback
//   st[ci] written by K2 (the region is mapped into every rank's GPU): active candidate ci is drainable (1) or
//          not (0)
constexpr size_t kShmHdr = 8;
enum ShmField {
  kShmCount = 0,          // input candidates of the call
  kShmBase = 1,           // its first local index + 1 (0: none)
  kShmFirstFallback = 2,  // first fallback (global) + 1
  kShmDone = 3,           // 1: the rank has finished this tick's walk
  kShmRankNext = 4        // smallest global index the rank has not planned after this call + 1 (0: none)
};
enum ShmInput : uint32_t { kInActive = 0, kInNoPods = 1, kInFallback = 2, kInCodeMask = 3 };

struct ShmSeg {
  uint64_t* host = nullptr;  // every rank's regions
  int32_t max_cand = 0;      // input candidates per rank and call
  int32_t nranks = 1, rank = 0;
  uint32_t session = 0;
};
inline size_t shm_region_words(int32_t max_cand) { return kShmHdr + 2 * static_cast<size_t>(max_cand); }
inline uint64_t* shm_region(const ShmSeg& s, int32_t r, int p) {
  return s.host + (static_cast<size_t>(r) * 2 + static_cast<size_t>(p)) * shm_region_words(s.max_cand);
}
// tags of the shared words: the high bit set, so they never equal a single-rank run's in the context's private
// result words
inline uint32_t shm_tag(uint32_t session, uint64_t tick) { return (session + static_cast<uint32_t>(tick)) | 0x80000000u; }

// Before K2, the host half of tick `tick` (from 1): once every rank has finished walking tick - 2, which used the
// region of this parity before, this rank's input words, a release fence and its header.  K2 then writes the
// outcome words at stat (a pointer into the segment).  base: the call's first local candidate; first_fallback:
// global, -1 none; rank_next: ~0 none.
struct ShmPublished {
  WordsStatus st = kWordsOk;
  int p = 0;
  uint32_t tag = 0;
  uint64_t* stat = nullptr;
};
ShmPublished shm_publish(const ShmSeg& s, uint64_t tick, const CandView& c, int32_t base, int32_t first_fallback,
                         uint64_t rank_next, ResultWait& wait);

// After K2: every rank's words in global candidate order (rank g % N holds global index g) -- every index some
// rank planned in this call, ascending (the ranks' first local indices may differ: a merge, so an index no rank
// planned is skipped), up to the first drainable one: what allreduce(min) + K3 give (rescheduler.go:280-286
// stops at the first drainable candidate, whichever rank planned it).  Marks this rank's walk of the tick done
// and writes `res` as K3 would, the owner's mapping from own_map (its K2's res_map words, by active pod).
WordsStatus shm_reduce(const ShmSeg& s, int p, uint32_t tag, const CandView& c, const volatile uint64_t* own_map,
                       volatile uint64_t* res, int32_t n_header, ResultWait& wait);

}  // namespace sr
