// podstore.inc — the pod cache's store: uid -> entry in C++, no Python.
// Unity-build fragment, #included into kwcore.cpp inside its anonymous
// namespace just before podcache.inc (the _kwcore.PodCache bindings over it),
// and into check/podstore_check.cpp on its own (scripts/podstore_check.sh).
//
// One entry per live pod, as ops/cache.py's PodCache holds it: keys and names
// are std::strings, namespaces and phases are interned to small ids
// (0 = None), and the payload core is kept as raw bytes. An entry's alert
// state is addressed by kind: a "last signature" slot per SigKind and a timer
// per TimerKind. A new alert adds an enum member here; nothing below names a
// kind except the one rule in PodStore::set_timer.

// The payload core is immutable once stored and shared by reference: a
// checkpoint snapshot (checkpoint.inc) keeps the cores of the moment without
// copying them, and a later event replaces the pointer, never the bytes.
using CoreRef = std::shared_ptr<const std::string>;

// The signature of a pod's findings at its last event (findings.inc), 0 for
// none: container failures (watcher.alerts.container_failures), condition
// findings (pod_conditions), and 1 while its graceful deletion has begun
// (terminating). In memory only: not in checkpoints or hand-over records.
enum SigKind { SIG_FAIL, SIG_COND, SIG_TERM, N_SIG };

// A time the overdue sweep measures from (seconds since the epoch,
// findings.inc): the deletion deadline of a terminating pod
// (watcher.alerts.terminating_overdue_seconds) and the creation time of a pod
// still Pending (pending_overdue_seconds) and the time the Ready condition of
// a Running pod turned False (unready_overdue_seconds). In memory only, like
// the signatures.
enum TimerKind { TIMER_DEADLINE, TIMER_PENDING, TIMER_UNREADY, N_TIMER };

// The kinds that keep cores: the filters may send none of such a pod's lines,
// so the core of an unsent line is kept for the sweep to report from, and lives
// as long as the timer. The two exclude each other by phase.
constexpr bool timer_keeps_core(TimerKind k) { return k == TIMER_PENDING || k == TIMER_UNREADY; }

struct CacheEntry {
    std::string rv, name;
    CoreRef core;  // nullptr: never notified
    uint32_t ns_id = 0, phase_id = 0;  // 0 = None
    uint32_t list_gen = 0;  // the relist (relist.inc) that last saw this pod in a LIST
    bool rv_none = false, name_none = false;
    // `core` is that of an unsent Pending or Running-but-unready line, kept for
    // the sweep to report from; it goes when the timer of that kind (one that
    // keeps cores) goes, and a send replaces it.
    bool core_kept = false;
    // Per timer kind: whether the entry has one (timer[k].at is meaningful
    // then) and whether the sweep reported it — a mark per kind, so a pod
    // reported pending-overdue is still reported termination-overdue. Written
    // through PodStore::set_timer only, which keeps the timed lists. (Apart
    // from the timers, with the other flags: a record per kind would pad.)
    bool timed[N_TIMER] = {}, reported[N_TIMER] = {};
    uint64_t sig[N_SIG] = {};
    struct Timer {
        int64_t at = 0;
        CacheEntry* prev = nullptr;  // links in the shard's list of this kind, while timed
        CacheEntry* next = nullptr;
    } timer[N_TIMER];
    // Managed by PodStore: this entry's uid (the map node's key — unordered_map
    // nodes never move) and its links in the per-namespace list.
    const std::string* key = nullptr;
    CacheEntry* ns_prev = nullptr;
    CacheEntry* ns_next = nullptr;
};
#if defined(__x86_64__) && defined(__GLIBCXX__)
// 200 bytes with three signatures and two timers; the unready timer added 24
// (its two flag bytes fit the padding): 2.4 MB per 100k pods. At 100k pods a
// word more per entry is 800 KB.
static_assert(sizeof(CacheEntry) <= 224, "CacheEntry grew");
#endif

// Hash for string-keyed maps that also finds by std::string_view (C++20
// heterogeneous lookup): the pipeline looks keys up straight from the watch
// buffer and builds a std::string only for an insertion.
// A key whose hash was computed elsewhere: the decode workers hash each
// event's uid and namespace while the line is hot in their cache, so the
// event-loop thread's lookups (apply_line) skip hashing.
struct HashedView {
    std::string_view s;
    size_t h;
};
inline bool operator==(const std::string& a, const HashedView& b) noexcept { return std::string_view(a) == b.s; }
inline bool operator==(const HashedView& a, const std::string& b) noexcept { return a.s == std::string_view(b); }

inline size_t sv_hash(std::string_view s) noexcept { return std::hash<std::string_view>{}(s); }

struct SvHash {
    using is_transparent = void;
    size_t operator()(std::string_view s) const noexcept { return sv_hash(s); }
    size_t operator()(const HashedView& k) const noexcept { return k.h; }
};
template <class V>
using SvMap = std::unordered_map<std::string, V, SvHash, std::equal_to<>>;

// uid -> entry, plus every entry threaded on an intrusive list per namespace
// id, so the namespace-scoped work (a scope's relist sweep, dropping the
// namespaces a shard gave up, counting a deleted namespace's pods) touches
// only that namespace's entries instead of walking the whole cache. Every
// insertion and erasure goes through here to keep the lists exact. The entries
// that have a timer are threaded on one more list per shard and kind, the
// timed list: an overdue sweep walks the pods it is about, not the cache.
//
// The store is split into SHARDS tables by the uid's hash, each with its own
// lists: a batch's events are applied by several threads at once
// (engine.inc, partitioned apply), each owning whole shards for the batch —
// every event of one pod lands in one shard, so per-pod order is the stream
// order and no two threads touch one table. Outside a batch only the
// event-loop thread uses the store, across all shards.
class PodStore {
  public:
    static constexpr uint32_t SHARDS = 16;
    using Map = SvMap<CacheEntry>;
    struct Shard {
        Map map;
        std::vector<CacheEntry*> heads;
        std::vector<size_t> counts;
        CacheEntry* timed_head[N_TIMER] = {};  // the timed lists: entries with a timer of that kind
        size_t timed_count[N_TIMER] = {};
    };
    // The shard of a uid hash (sv_hash): its top bits (the map's buckets use the low ones).
    static uint32_t shard_of(size_t h) noexcept { return (uint32_t)(h >> 58) & (SHARDS - 1); }

    struct iterator {
        Shard* sh = nullptr;
        Map::iterator it;
        std::pair<const std::string, CacheEntry>* operator->() const { return &*it; }
        std::pair<const std::string, CacheEntry>& operator*() const { return *it; }
        bool operator==(const iterator& o) const { return sh == o.sh && (!sh || it == o.it); }
        bool operator!=(const iterator& o) const { return !(*this == o); }
    };

    size_t size() const {
        size_t n = 0;
        for (const Shard& s : shards_) n += s.map.size();
        return n;
    }
    iterator end() { return iterator{}; }
    iterator find(std::string_view k) { return find(HashedView{k, sv_hash(k)}); }
    iterator find(const HashedView& k) {
        Shard& s = shards_[shard_of(k.h)];
        auto it = s.map.find(k);
        return it == s.map.end() ? iterator{} : iterator{&s, it};
    }

    // The entry for k, created empty in namespace ns_id if absent.
    CacheEntry& emplace(std::string_view k, uint32_t ns_id, bool& inserted) {
        return emplace(HashedView{k, sv_hash(k)}, ns_id, inserted);
    }
    CacheEntry& emplace(const HashedView& k, uint32_t ns_id, bool& inserted) {
        Shard& s = shards_[shard_of(k.h)];
        auto r = s.map.try_emplace(std::string(k.s));
        inserted = r.second;
        CacheEntry& e = r.first->second;
        if (inserted) {
            e.key = &r.first->first;
            e.ns_id = ns_id;
            link(s, e);
        }
        return e;
    }
    void set_ns(CacheEntry& e, uint32_t ns_id) {
        if (e.ns_id == ns_id) return;
        Shard& s = shard_for(e);
        unlink(s, e);
        e.ns_id = ns_id;
        link(s, e);
    }
    void erase(iterator it) {
        CacheEntry& e = it.it->second;
        unlink(*it.sh, e);
        for (int k = 0; k < N_TIMER; ++k)
            if (e.timed[k]) untrack((TimerKind)k, *it.sh, e);
        it.sh->map.erase(it.it);
    }
    bool erase(std::string_view k) {
        auto it = find(k);
        if (it == end()) return false;
        erase(it);
        return true;
    }
    void clear() {
        for (Shard& s : shards_) s = Shard();
    }
    // The timer of kind k of e, an entry of the shard `it` found (or its key
    // hashes to). Without a value it clears the timer and its reported mark;
    // a value keeps the mark: a timer that moves does not re-alert. Within a
    // partitioned batch the caller owns e's shard, so no lock is needed.
    void set_timer(TimerKind k, iterator it, bool has, int64_t at) { set_timer(k, *it.sh, it.it->second, has, at); }
    void set_timer(TimerKind k, CacheEntry& e, bool has, int64_t at) {
        if (!has && !e.timed[k] && !e.core_kept) return;
        set_timer(k, shard_for(e), e, has, at);
    }
    // entries with a timer of kind k
    size_t timed(TimerKind k) const {
        size_t n = 0;
        for (const Shard& s : shards_) n += s.timed_count[k];
        return n;
    }
    // every entry with a timer of kind k (any order); fn must not erase or untrack
    template <class F>
    void for_each_timed(TimerKind k, F&& fn) {
        for (Shard& s : shards_)
            for (CacheEntry* e = s.timed_head[k]; e; e = e->timer[k].next) fn(*e);
    }
    void reserve(size_t n) {
        for (Shard& s : shards_) s.map.reserve(s.map.size() + n / SHARDS + 1);
    }
    // every entry (any order): fn(const std::string& uid, CacheEntry&)
    template <class F>
    void for_each(F&& fn) {
        for (Shard& s : shards_)
            for (auto& kv : s.map) fn(kv.first, kv.second);
    }
    // every entry of namespace ns_id (any order); fn must not erase other
    // entries of that namespace (it may erase the one it is given)
    template <class F>
    void for_each_in(uint32_t ns_id, F&& fn) {
        for (Shard& s : shards_) {
            CacheEntry* e = ns_id < s.heads.size() ? s.heads[ns_id] : nullptr;
            while (e) {
                CacheEntry* next = e->ns_next;
                fn(*e);
                e = next;
            }
        }
    }
    // some entry of namespace ns_id, or nullptr
    CacheEntry* any_in(uint32_t ns_id) const {
        for (const Shard& s : shards_)
            if (ns_id < s.heads.size() && s.heads[ns_id]) return s.heads[ns_id];
        return nullptr;
    }
    Map& shard_map(uint32_t i) { return shards_[i].map; }
    size_t count(uint32_t ns_id) const {
        size_t n = 0;
        for (const Shard& s : shards_) n += ns_id < s.counts.size() ? s.counts[ns_id] : 0;
        return n;
    }
    uint32_t ns_ids() const {
        size_t n = 0;
        for (const Shard& s : shards_) n = std::max(n, s.heads.size());
        return (uint32_t)n;
    }

  private:
    Shard shards_[SHARDS];
    Shard& shard_for(const CacheEntry& e) { return shards_[shard_of(sv_hash(*e.key))]; }
    static void set_timer(TimerKind k, Shard& s, CacheEntry& e, bool has, int64_t at) {
        CacheEntry::Timer& t = e.timer[k];
        if (!has) {
            if (e.timed[k]) untrack(k, s, e);
            e.reported[k] = false;
            // the one rule that depends on the kind: the core of a line
            // nobody sent lives as long as the timer of a kind that keeps cores
            // (the other such kind's, if a line just set it, holds the core on)
            if (timer_keeps_core(k) && e.core_kept && !(e.timed[TIMER_PENDING] || e.timed[TIMER_UNREADY])) {
                e.core.reset();
                e.core_kept = false;
            }
            return;
        }
        if (!e.timed[k]) {
            e.timed[k] = true;
            t.prev = nullptr;
            t.next = s.timed_head[k];
            if (t.next) t.next->timer[k].prev = &e;
            s.timed_head[k] = &e;
            ++s.timed_count[k];
        }
        t.at = at;
    }
    static void untrack(TimerKind k, Shard& s, CacheEntry& e) {
        CacheEntry::Timer& t = e.timer[k];
        if (t.prev) t.prev->timer[k].next = t.next; else s.timed_head[k] = t.next;
        if (t.next) t.next->timer[k].prev = t.prev;
        t.prev = t.next = nullptr;
        e.timed[k] = false;
        --s.timed_count[k];
    }
    static void link(Shard& s, CacheEntry& e) {
        const uint32_t n = e.ns_id;
        if (n >= s.heads.size()) {
            s.heads.resize(n + 1, nullptr);
            s.counts.resize(n + 1, 0);
        }
        e.ns_prev = nullptr;
        e.ns_next = s.heads[n];
        if (e.ns_next) e.ns_next->ns_prev = &e;
        s.heads[n] = &e;
        ++s.counts[n];
    }
    static void unlink(Shard& s, CacheEntry& e) {
        if (e.ns_prev) e.ns_prev->ns_next = e.ns_next; else s.heads[e.ns_id] = e.ns_next;
        if (e.ns_next) e.ns_next->ns_prev = e.ns_prev;
        e.ns_prev = e.ns_next = nullptr;
        --s.counts[e.ns_id];
    }
};

// The entries a sweep of kind k at now_s reports: after_s or more past their
// timer, not yet reported as that, with a payload core, of namespace id
// scope_ns when scoped. Each is marked reported. Walks the timed lists only.
inline void store_take_due(PodStore& st, TimerKind k, int64_t now_s, int64_t after_s, bool scoped, uint32_t scope_ns,
                           std::vector<CacheEntry*>& out) {
    st.for_each_timed(k, [&](CacheEntry& e) {
        if (e.reported[k] || !e.core || (scoped && e.ns_id != scope_ns)) return;
        // (the timer is any int64 a caller stored: compare without overflow)
        if ((__int128)now_s - (__int128)e.timer[k].at < (__int128)after_s) return;
        e.reported[k] = true;
        out.push_back(&e);
    });
}

// Replace every field of the entry for `key` (created if absent) with `e`'s:
// a whole new entry, nothing known of its containers, conditions or deletion.
inline void store_put(PodStore& st, std::string_view key, CacheEntry&& e) {
    bool inserted;
    CacheEntry& d = st.emplace(key, e.ns_id, inserted);
    st.set_ns(d, e.ns_id);
    d.rv = std::move(e.rv);
    d.name = std::move(e.name);
    // (the timers before the core: a kept one goes with its timer)
    for (int k = 0; k < N_TIMER; ++k) st.set_timer((TimerKind)k, d, false, 0);
    d.core = std::move(e.core);
    d.phase_id = e.phase_id;
    d.rv_none = e.rv_none;
    d.name_none = e.name_none;
    for (uint64_t& s : d.sig) s = 0;
}
