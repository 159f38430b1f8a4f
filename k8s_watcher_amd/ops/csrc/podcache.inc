// podcache.inc — native pod cache (_kwcore.PodCache). Unity-build fragment,
// #included into kwcore.cpp inside its anonymous namespace before engine.inc.
//
// Same contents and semantics as ops/cache.py's PodCache — one entry per live
// pod, uid -> [resourceVersion, phase, namespace, name, core] — but held in
// C++ so the fused Pipeline updates it without creating a Python object per
// event: keys and names are std::strings, namespaces and phases are interned
// to small ids (0 = None), and the payload core is kept as raw bytes. The
// Python side (reconcile, checkpoint, tests) reaches it through the methods
// below, which convert on the way out.

// The payload core is immutable once stored and shared by reference: a
// checkpoint snapshot (checkpoint.inc) keeps the cores of the moment without
// copying them, and a later event replaces the pointer, never the bytes.
using CoreRef = std::shared_ptr<const std::string>;

struct CacheEntry {
    std::string rv, name;
    CoreRef core;  // nullptr: never notified
    uint32_t ns_id = 0, phase_id = 0;  // 0 = None
    bool rv_none = false, name_none = false;
    uint32_t list_gen = 0;  // the relist (relist.inc) that last saw this pod in a LIST
    // watcher.alerts.container_failures: the signature of the pod's findings
    // at its last event (findings.inc), 0 for none. In memory only: not in
    // checkpoints or hand-over records.
    uint64_t fail_sig = 0;
    // watcher.alerts.pod_conditions: the signature of the pod's condition
    // findings at its last event, 0 for none. In memory only, like fail_sig.
    uint64_t cond_sig = 0;
    // watcher.alerts.terminating: 1 when the pod's graceful deletion had begun
    // at its last event, else 0. In memory only, like the two above.
    uint64_t term_sig = 0;
    // watcher.alerts.terminating_overdue_seconds: the pod's deletion deadline
    // (seconds since the epoch, findings.inc; meaningful while has_deadline)
    // and whether the overdue sweep reported it. In memory only, like the
    // signatures. Written through PodStore::set_deadline only, which keeps the
    // tracked list.
    int64_t deadline = 0;
    bool has_deadline = false, reported = false;
    // watcher.alerts.pending_overdue_seconds: the creation time of a pod that
    // is still Pending (findings.inc pending_since; meaningful while
    // has_pending) and whether the sweep reported it: a mark of its own, so a
    // pod reported pending-overdue is still reported termination-overdue.
    // In memory only; written through PodStore::set_pending only. core_kept:
    // `core` is that of an unsent Pending line, kept for the sweep to report
    // from; it goes when the pending-since goes, and a send replaces it.
    bool has_pending = false, pend_reported = false, core_kept = false;
    int64_t pend_since = 0;
    // Managed by PodStore: this entry's uid (the map node's key — unordered_map
    // nodes never move), its links in the per-namespace list and, while it has
    // a deadline, in its shard's tracked list.
    const std::string* key = nullptr;
    CacheEntry* ns_prev = nullptr;
    CacheEntry* ns_next = nullptr;
    CacheEntry* due_prev = nullptr;
    CacheEntry* due_next = nullptr;
    CacheEntry* pend_prev = nullptr;  // ... and, while it has a pending-since, in the shard's pending list
    CacheEntry* pend_next = nullptr;
};

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
// that have a deletion deadline are threaded on one more list per shard, the
// tracked list: the overdue sweep walks the terminating pods, not the cache.
//
// The store is split into SHARDS tables by the uid's hash, each with its own
// namespace lists: a batch's events are applied by several threads at once
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
        CacheEntry* due_head = nullptr;  // the tracked list: entries with a deadline
        size_t due_count = 0;
        CacheEntry* pend_head = nullptr;  // the pending list: entries with a pending-since
        size_t pend_count = 0;
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
        Shard& s = shards_[shard_of(sv_hash(*e.key))];
        unlink(s, e);
        e.ns_id = ns_id;
        link(s, e);
    }
    void erase(iterator it) {
        unlink(*it.sh, it.it->second);
        if (it.it->second.has_deadline) untrack(*it.sh, it.it->second);
        if (it.it->second.has_pending) untrack_pending(*it.sh, it.it->second);
        it.sh->map.erase(it.it);
    }
    bool erase(std::string_view k) {
        auto it = find(k);
        if (it == end()) return false;
        erase(it);
        return true;
    }
    void clear() {
        for (Shard& s : shards_) {
            s.map.clear();
            s.heads.clear();
            s.counts.clear();
            s.due_head = s.pend_head = nullptr;
            s.due_count = s.pend_count = 0;
        }
    }
    // The deadline of e, an entry of the shard `it` found (or its key hashes
    // to). None clears the deadline and the reported mark; a value keeps the
    // mark: a deadline that moves does not re-alert. Within a partitioned
    // batch the caller owns e's shard, so no lock is needed.
    void set_deadline(iterator it, bool has, int64_t due) { set_deadline(*it.sh, it.it->second, has, due); }
    void set_deadline(CacheEntry& e, bool has, int64_t due) {
        if (!has && !e.has_deadline) return;
        set_deadline(shards_[shard_of(sv_hash(*e.key))], e, has, due);
    }
    size_t tracked() const {
        size_t n = 0;
        for (const Shard& s : shards_) n += s.due_count;
        return n;
    }
    // every entry with a deadline (any order); fn must not erase or untrack
    template <class F>
    void for_each_tracked(F&& fn) {
        for (Shard& s : shards_)
            for (CacheEntry* e = s.due_head; e; e = e->due_next) fn(*e);
    }
    // The pending-since of e, as set_deadline: None clears it, its reported
    // mark and a kept core; a value keeps the mark.
    void set_pending(iterator it, bool has, int64_t since) { set_pending(*it.sh, it.it->second, has, since); }
    void set_pending(CacheEntry& e, bool has, int64_t since) {
        if (!has && !e.has_pending && !e.core_kept) return;
        set_pending(shards_[shard_of(sv_hash(*e.key))], e, has, since);
    }
    size_t pending_tracked() const {
        size_t n = 0;
        for (const Shard& s : shards_) n += s.pend_count;
        return n;
    }
    // every entry with a pending-since (any order); fn must not erase or untrack
    template <class F>
    void for_each_pending(F&& fn) {
        for (Shard& s : shards_)
            for (CacheEntry* e = s.pend_head; e; e = e->pend_next) fn(*e);
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
    static void set_deadline(Shard& s, CacheEntry& e, bool has, int64_t due) {
        if (!has) {
            if (e.has_deadline) untrack(s, e);
            e.reported = false;
            return;
        }
        if (!e.has_deadline) {
            e.has_deadline = true;
            e.due_prev = nullptr;
            e.due_next = s.due_head;
            if (e.due_next) e.due_next->due_prev = &e;
            s.due_head = &e;
            ++s.due_count;
        }
        e.deadline = due;
    }
    static void untrack(Shard& s, CacheEntry& e) {
        if (e.due_prev) e.due_prev->due_next = e.due_next; else s.due_head = e.due_next;
        if (e.due_next) e.due_next->due_prev = e.due_prev;
        e.due_prev = e.due_next = nullptr;
        e.has_deadline = false;
        --s.due_count;
    }
    static void set_pending(Shard& s, CacheEntry& e, bool has, int64_t since) {
        if (!has) {
            if (e.has_pending) untrack_pending(s, e);
            e.pend_reported = false;
            if (e.core_kept) {  // the core of a line nobody sent: it lives as long as the pending-since
                e.core.reset();
                e.core_kept = false;
            }
            return;
        }
        if (!e.has_pending) {
            e.has_pending = true;
            e.pend_prev = nullptr;
            e.pend_next = s.pend_head;
            if (e.pend_next) e.pend_next->pend_prev = &e;
            s.pend_head = &e;
            ++s.pend_count;
        }
        e.pend_since = since;
    }
    static void untrack_pending(Shard& s, CacheEntry& e) {
        if (e.pend_prev) e.pend_prev->pend_next = e.pend_next; else s.pend_head = e.pend_next;
        if (e.pend_next) e.pend_next->pend_prev = e.pend_prev;
        e.pend_prev = e.pend_next = nullptr;
        e.has_pending = false;
        --s.pend_count;
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

// String <-> small id, with the Python str for each id created on first use.
struct IdTable {
    std::vector<std::string> text{std::string()};  // id 0 = None
    std::vector<PyObject*> objs{nullptr};
    SvMap<uint32_t> ids;
    ~IdTable() {
        for (PyObject* o : objs) Py_XDECREF(o);
    }
    uint32_t intern(std::string_view s) { return intern(HashedView{s, 0}, false); }
    // hashed: k.h is sv_hash(k.s) (computed by a decode worker)
    uint32_t intern(const HashedView& k, bool hashed) {
        const std::string_view s = k.s;
        if (text.size() <= 9) {  // a handful (pod phases): a scan beats hashing
            for (uint32_t i = 1; i < (uint32_t)text.size(); ++i)
                if (text[i].size() == s.size() && std::memcmp(text[i].data(), s.data(), s.size()) == 0) return i;
        } else {
            auto it = hashed ? ids.find(k) : ids.find(s);
            if (it != ids.end()) return it->second;
        }
        uint32_t id = (uint32_t)text.size();
        text.emplace_back(s);
        objs.push_back(nullptr);
        ids.emplace(std::string(s), id);
        return id;
    }
    // id of k without inserting it (UINT32_MAX: never interned). Read-only:
    // safe from several threads while nothing interns (the partitioned apply).
    uint32_t lookup(const HashedView& k, bool hashed) const {
        const std::string_view s = k.s;
        if (text.size() <= 9) {
            for (uint32_t i = 1; i < (uint32_t)text.size(); ++i)
                if (text[i].size() == s.size() && std::memcmp(text[i].data(), s.data(), s.size()) == 0) return i;
            return UINT32_MAX;
        }
        auto it = hashed ? ids.find(k) : ids.find(s);
        return it == ids.end() ? UINT32_MAX : it->second;
    }
    // new reference (None for id 0)
    PyObject* py(uint32_t id) {
        if (id == 0) Py_RETURN_NONE;
        if (!objs[id]) {
            objs[id] = PyUnicode_DecodeUTF8(text[id].data(), (Py_ssize_t)text[id].size(), "replace");
            if (!objs[id]) return nullptr;
        }
        Py_INCREF(objs[id]);
        return objs[id];
    }
};

struct PodCacheObject {
    PyObject_HEAD
    PodStore* store;
    IdTable* ns;
    IdTable* phases;
    PyObject* missing;  // sentinel returned by observe() for unknown pods
};

// uid None (a pod without metadata.uid) gets a key no JSON string decodes to
// by accident in practice: a lone NUL byte followed by a marker.
const std::string NONE_UID("\0<none>", 7);

// Python value (str or None) -> UTF-8 text; false + TypeError otherwise.
bool opt_text(PyObject* o, std::string& out, bool& none) {
    if (o == Py_None) {
        out.clear();
        none = true;
        return true;
    }
    none = false;
    if (!PyUnicode_Check(o)) {
        PyErr_SetString(PyExc_TypeError, "expected str or None");
        return false;
    }
    Py_ssize_t n;
    const char* u = PyUnicode_AsUTF8AndSize(o, &n);
    if (!u) return false;
    out.assign(u, (size_t)n);
    return true;
}

bool uid_key(PyObject* o, std::string& out) {
    bool none;
    if (!opt_text(o, out, none)) return false;
    if (none) out = NONE_UID;
    return true;
}

PyObject* key_py(const std::string& k) {
    if (k == NONE_UID) Py_RETURN_NONE;
    return PyUnicode_DecodeUTF8(k.data(), (Py_ssize_t)k.size(), "replace");
}

uint32_t intern_opt(IdTable* t, PyObject* o, bool& ok) {
    std::string s;
    bool none;
    ok = opt_text(o, s, none);
    if (!ok || none) return 0;
    return t->intern(s);
}

PyObject* opt_py(const std::string& s, bool none) {
    if (none) Py_RETURN_NONE;
    return PyUnicode_DecodeUTF8(s.data(), (Py_ssize_t)s.size(), "replace");
}

// [rv, phase, ns, name, core] as a fresh list
PyObject* entry_list(PodCacheObject* self, const CacheEntry& e) {
    PyObject* core = e.core ? PyBytes_FromStringAndSize(e.core->data(), (Py_ssize_t)e.core->size())
                            : (Py_INCREF(Py_None), Py_None);
    return Py_BuildValue("[NNNNN]", opt_py(e.rv, e.rv_none), self->phases->py(e.phase_id), self->ns->py(e.ns_id),
                         opt_py(e.name, e.name_none), core);
}

PyObject* PodCache_new(PyTypeObject* type, PyObject*, PyObject*) {
    PodCacheObject* self = (PodCacheObject*)type->tp_alloc(type, 0);
    if (!self) return nullptr;
    self->store = new PodStore();
    self->ns = new IdTable();
    self->phases = new IdTable();
    self->missing = nullptr;
    return (PyObject*)self;
}

int PodCache_init(PodCacheObject* self, PyObject* args, PyObject*) {
    PyObject* missing = Py_None;
    if (!PyArg_ParseTuple(args, "|O", &missing)) return -1;
    Py_INCREF(missing);
    Py_XSETREF(self->missing, missing);
    return 0;
}

void PodCache_dealloc(PodCacheObject* self) {
    delete self->store;
    delete self->ns;
    delete self->phases;
    Py_XDECREF(self->missing);
    Py_TYPE(self)->tp_free((PyObject*)self);
}

Py_ssize_t PodCache_len(PodCacheObject* self) { return (Py_ssize_t)self->store->size(); }

int PodCache_contains(PodCacheObject* self, PyObject* uid) {
    std::string k;
    if (!uid_key(uid, k)) return -1;
    return self->store->find(k) != self->store->end() ? 1 : 0;
}

PyObject* PodCache_get(PodCacheObject* self, PyObject* uid) {
    std::string k;
    if (!uid_key(uid, k)) return nullptr;
    auto it = self->store->find(k);
    if (it == self->store->end()) Py_RETURN_NONE;
    return entry_list(self, it->second);
}

// observe(etype, uid, rv, phase, ns, name) -> previous phase or the MISSING sentinel
PyObject* PodCache_observe(PodCacheObject* self, PyObject* args) {
    const char* et;
    PyObject *uid, *rv, *phase, *ns, *name;
    if (!PyArg_ParseTuple(args, "sOOOOO", &et, &uid, &rv, &phase, &ns, &name)) return nullptr;
    std::string k;
    if (!uid_key(uid, k)) return nullptr;
    PodStore& st = *self->store;
    auto it = st.find(k);
    PyObject* prev;
    if (it == st.end()) {
        prev = self->missing;
        Py_INCREF(prev);
    } else {
        prev = self->phases->py(it->second.phase_id);
        if (!prev) return nullptr;
    }
    bool ok = true;
    if (std::strcmp(et, "DELETED") == 0) {
        if (it != st.end()) st.erase(it);
        return prev;
    }
    uint32_t pid = intern_opt(self->phases, phase, ok);
    if (!ok) goto bad;
    {
        CacheEntry* e;
        if (it == st.end()) {
            std::string name_text;
            bool name_none;
            const uint32_t ns_id = intern_opt(self->ns, ns, ok);
            if (!ok || !opt_text(name, name_text, name_none)) goto bad;
            bool inserted;
            e = &st.emplace(k, ns_id, inserted);
            e->name = std::move(name_text);
            e->name_none = name_none;
        } else {
            e = &it->second;
        }
        if (!opt_text(rv, e->rv, e->rv_none)) goto bad;
        e->phase_id = pid;
    }
    return prev;
bad:
    Py_DECREF(prev);
    return nullptr;
}

PyObject* PodCache_set_core(PodCacheObject* self, PyObject* args) {
    PyObject* uid;
    Py_buffer core;
    if (!PyArg_ParseTuple(args, "Oy*", &uid, &core)) return nullptr;
    std::string k;
    bool ok = uid_key(uid, k);
    if (ok) {
        auto it = self->store->find(k);
        if (it != self->store->end()) {
            it->second.core = std::make_shared<const std::string>((const char*)core.buf, (size_t)core.len);
            it->second.core_kept = false;
        }
    }
    PyBuffer_Release(&core);
    if (!ok) return nullptr;
    Py_RETURN_NONE;
}

// keep_core(uid, core): the payload core of an unsent Pending line
// (watcher.alerts.pending_overdue_seconds), marked as kept, not sent: clearing
// the pending-since drops it, set_core replaces it. A pod not cached stores nothing.
PyObject* PodCache_keep_core(PodCacheObject* self, PyObject* args) {
    PyObject* uid;
    Py_buffer core;
    if (!PyArg_ParseTuple(args, "Oy*", &uid, &core)) return nullptr;
    std::string k;
    bool ok = uid_key(uid, k);
    if (ok) {
        auto it = self->store->find(k);
        if (it != self->store->end()) {
            it->second.core = std::make_shared<const std::string>((const char*)core.buf, (size_t)core.len);
            it->second.core_kept = true;
        }
    }
    PyBuffer_Release(&core);
    if (!ok) return nullptr;
    Py_RETURN_NONE;
}

// core_kept(uid) -> whether the pod's core is a kept one
PyObject* PodCache_core_kept(PodCacheObject* self, PyObject* uid) {
    std::string k;
    if (!uid_key(uid, k)) return nullptr;
    auto it = self->store->find(k);
    return PyBool_FromLong(it != self->store->end() && it->second.core_kept);
}

// swap_failure(uid, signature) -> the pod's previous failure signature (0 for
// none, and for a pod not cached, which stores nothing)
PyObject* PodCache_swap_failure(PodCacheObject* self, PyObject* args) {
    PyObject* uid;
    unsigned long long sig;
    if (!PyArg_ParseTuple(args, "OK", &uid, &sig)) return nullptr;
    std::string k;
    if (!uid_key(uid, k)) return nullptr;
    auto it = self->store->find(k);
    unsigned long long prev = 0;
    if (it != self->store->end()) {
        prev = it->second.fail_sig;
        it->second.fail_sig = sig;
    }
    return PyLong_FromUnsignedLongLong(prev);
}

// swap_condition(uid, signature) -> the pod's previous condition signature,
// as swap_failure; the two are independent
PyObject* PodCache_swap_condition(PodCacheObject* self, PyObject* args) {
    PyObject* uid;
    unsigned long long sig;
    if (!PyArg_ParseTuple(args, "OK", &uid, &sig)) return nullptr;
    std::string k;
    if (!uid_key(uid, k)) return nullptr;
    auto it = self->store->find(k);
    unsigned long long prev = 0;
    if (it != self->store->end()) {
        prev = it->second.cond_sig;
        it->second.cond_sig = sig;
    }
    return PyLong_FromUnsignedLongLong(prev);
}

// swap_terminating(uid, signature) -> the pod's previous terminating
// signature, as swap_failure; independent of the other two
PyObject* PodCache_swap_terminating(PodCacheObject* self, PyObject* args) {
    PyObject* uid;
    unsigned long long sig;
    if (!PyArg_ParseTuple(args, "OK", &uid, &sig)) return nullptr;
    std::string k;
    if (!uid_key(uid, k)) return nullptr;
    auto it = self->store->find(k);
    unsigned long long prev = 0;
    if (it != self->store->end()) {
        prev = it->second.term_sig;
        it->second.term_sig = sig;
    }
    return PyLong_FromUnsignedLongLong(prev);
}

// set_deadline(uid, due | None): the pod's deletion deadline. None clears it
// and the reported mark, a value keeps the mark; an unknown uid is a no-op.
PyObject* PodCache_set_deadline(PodCacheObject* self, PyObject* args) {
    PyObject *uid, *due;
    if (!PyArg_ParseTuple(args, "OO", &uid, &due)) return nullptr;
    std::string k;
    if (!uid_key(uid, k)) return nullptr;
    long long d = 0;
    if (due != Py_None) {
        d = PyLong_AsLongLong(due);
        if (d == -1 && PyErr_Occurred()) return nullptr;
    }
    auto it = self->store->find(k);
    if (it != self->store->end()) self->store->set_deadline(it, due != Py_None, (int64_t)d);
    Py_RETURN_NONE;
}

// deadline(uid) -> the pod's deadline or None
PyObject* PodCache_deadline(PodCacheObject* self, PyObject* uid) {
    std::string k;
    if (!uid_key(uid, k)) return nullptr;
    auto it = self->store->find(k);
    if (it == self->store->end() || !it->second.has_deadline) Py_RETURN_NONE;
    return PyLong_FromLongLong((long long)it->second.deadline);
}

// tracked() -> entries with a deadline
PyObject* PodCache_tracked(PodCacheObject* self, PyObject*) {
    return PyLong_FromSize_t(self->store->tracked());
}

// The entries a sweep at now_s reports: after_s or more past their deadline,
// not yet reported, with a payload core, of namespace id scope_ns when scoped.
// Each is marked reported. Walks the tracked lists only.
void store_take_overdue(PodStore& st, int64_t now_s, int64_t after_s, bool scoped, uint32_t scope_ns,
                        std::vector<CacheEntry*>& out) {
    st.for_each_tracked([&](CacheEntry& e) {
        // (the deadline is any int64 a caller stored: compare without overflow)
        if (e.reported || !e.core || (scoped && e.ns_id != scope_ns)) return;
        if ((__int128)now_s - (__int128)e.deadline < (__int128)after_s) return;
        e.reported = true;
        out.push_back(&e);
    });
}

bool ns_lookup(PodCacheObject* self, PyObject* arg, uint32_t& id, bool& ok);

// take_overdue(now_s, after_s, scope_ns=None) -> [(uid, namespace, name, core, deadline), ...]
PyObject* PodCache_take_overdue(PodCacheObject* self, PyObject* args) {
    long long now_s, after_s;
    PyObject* scope = Py_None;
    if (!PyArg_ParseTuple(args, "LL|O", &now_s, &after_s, &scope)) return nullptr;
    uint32_t ns_id = 0;
    const bool scoped = scope != Py_None;
    if (scoped) {
        bool ok;
        if (!ns_lookup(self, scope, ns_id, ok)) {
            if (!ok) return nullptr;
            return PyList_New(0);  // a namespace never seen: no entry is in it
        }
    }
    std::vector<CacheEntry*> due;
    store_take_overdue(*self->store, now_s, after_s, scoped, ns_id, due);
    PyObject* out = PyList_New(0);
    if (!out) return nullptr;
    for (CacheEntry* e : due) {
        PyObject* t = Py_BuildValue("(NNNy#L)", key_py(*e->key), self->ns->py(e->ns_id), opt_py(e->name, e->name_none),
                                    e->core->data(), (Py_ssize_t)e->core->size(), (long long)e->deadline);
        if (!t || PyList_Append(out, t) < 0) {
            Py_XDECREF(t);
            Py_DECREF(out);
            return nullptr;
        }
        Py_DECREF(t);
    }
    return out;
}

// set_pending_since(uid, since | None): the creation time of a pod still
// Pending. None clears it, its reported mark and a kept core; a value keeps
// the mark; an unknown uid is a no-op.
PyObject* PodCache_set_pending_since(PodCacheObject* self, PyObject* args) {
    PyObject *uid, *since;
    if (!PyArg_ParseTuple(args, "OO", &uid, &since)) return nullptr;
    std::string k;
    if (!uid_key(uid, k)) return nullptr;
    long long d = 0;
    if (since != Py_None) {
        d = PyLong_AsLongLong(since);
        if (d == -1 && PyErr_Occurred()) return nullptr;
    }
    auto it = self->store->find(k);
    if (it != self->store->end()) self->store->set_pending(it, since != Py_None, (int64_t)d);
    Py_RETURN_NONE;
}

// pending_since(uid) -> the pod's pending-since or None
PyObject* PodCache_pending_since(PodCacheObject* self, PyObject* uid) {
    std::string k;
    if (!uid_key(uid, k)) return nullptr;
    auto it = self->store->find(k);
    if (it == self->store->end() || !it->second.has_pending) Py_RETURN_NONE;
    return PyLong_FromLongLong((long long)it->second.pend_since);
}

// pending_tracked() -> entries with a pending-since
PyObject* PodCache_pending_tracked(PodCacheObject* self, PyObject*) {
    return PyLong_FromSize_t(self->store->pending_tracked());
}

// As store_take_overdue, for the pods still Pending: after_s or more past their
// creation, with their own mark. Walks the pending lists only.
void store_take_pending_overdue(PodStore& st, int64_t now_s, int64_t after_s, bool scoped, uint32_t scope_ns,
                                std::vector<CacheEntry*>& out) {
    st.for_each_pending([&](CacheEntry& e) {
        if (e.pend_reported || !e.core || (scoped && e.ns_id != scope_ns)) return;
        if ((__int128)now_s - (__int128)e.pend_since < (__int128)after_s) return;
        e.pend_reported = true;
        out.push_back(&e);
    });
}

// take_pending_overdue(now_s, after_s, scope_ns=None) -> [(uid, namespace, name, core, since), ...]
PyObject* PodCache_take_pending_overdue(PodCacheObject* self, PyObject* args) {
    long long now_s, after_s;
    PyObject* scope = Py_None;
    if (!PyArg_ParseTuple(args, "LL|O", &now_s, &after_s, &scope)) return nullptr;
    uint32_t ns_id = 0;
    const bool scoped = scope != Py_None;
    if (scoped) {
        bool ok;
        if (!ns_lookup(self, scope, ns_id, ok)) {
            if (!ok) return nullptr;
            return PyList_New(0);  // a namespace never seen: no entry is in it
        }
    }
    std::vector<CacheEntry*> due;
    store_take_pending_overdue(*self->store, now_s, after_s, scoped, ns_id, due);
    PyObject* out = PyList_New(0);
    if (!out) return nullptr;
    for (CacheEntry* e : due) {
        PyObject* t = Py_BuildValue("(NNNy#L)", key_py(*e->key), self->ns->py(e->ns_id), opt_py(e->name, e->name_none),
                                    e->core->data(), (Py_ssize_t)e->core->size(), (long long)e->pend_since);
        if (!t || PyList_Append(out, t) < 0) {
            Py_XDECREF(t);
            Py_DECREF(out);
            return nullptr;
        }
        Py_DECREF(t);
    }
    return out;
}

// Replace every field of the entry for `key` (created if absent) with `e`'s.
void store_put(PodStore& st, std::string_view key, CacheEntry&& e) {
    bool inserted;
    CacheEntry& d = st.emplace(key, e.ns_id, inserted);
    st.set_ns(d, e.ns_id);
    d.rv = std::move(e.rv);
    d.name = std::move(e.name);
    st.set_pending(d, false, 0);  // (before the core: a kept one goes with it)
    d.core = std::move(e.core);
    d.phase_id = e.phase_id;
    d.rv_none = e.rv_none;
    d.name_none = e.name_none;
    d.fail_sig = d.cond_sig = d.term_sig = 0;  // a whole new entry: nothing known of its containers, conditions or deletion
    st.set_deadline(d, false, 0);
}

// put(uid, rv, phase, ns, name, core=None): insert or replace a whole entry
PyObject* PodCache_put(PodCacheObject* self, PyObject* args) {
    PyObject *uid, *rv, *phase, *ns, *name, *core = Py_None;
    if (!PyArg_ParseTuple(args, "OOOOO|O", &uid, &rv, &phase, &ns, &name, &core)) return nullptr;
    std::string k;
    if (!uid_key(uid, k)) return nullptr;
    CacheEntry e;
    bool ok = true;
    e.phase_id = intern_opt(self->phases, phase, ok);
    if (!ok) return nullptr;
    e.ns_id = intern_opt(self->ns, ns, ok);
    if (!ok || !opt_text(rv, e.rv, e.rv_none) || !opt_text(name, e.name, e.name_none)) return nullptr;
    if (core != Py_None) {
        char* b;
        Py_ssize_t n;
        if (PyBytes_AsStringAndSize(core, &b, &n) < 0) return nullptr;
        e.core = std::make_shared<const std::string>(b, (size_t)n);
    }
    store_put(*self->store, k, std::move(e));
    Py_RETURN_NONE;
}

PyObject* PodCache_pop(PodCacheObject* self, PyObject* args) {
    PyObject *uid, *dflt = Py_None;
    if (!PyArg_ParseTuple(args, "O|O", &uid, &dflt)) return nullptr;
    std::string k;
    if (!uid_key(uid, k)) return nullptr;
    auto it = self->store->find(k);
    if (it == self->store->end()) {
        Py_INCREF(dflt);
        return dflt;
    }
    PyObject* r = entry_list(self, it->second);
    self->store->erase(it);
    return r;
}

// items() -> [(uid, [rv, phase, ns, name, core]), ...] (a snapshot)
PyObject* PodCache_items(PodCacheObject* self, PyObject*) {
    PyObject* out = PyList_New((Py_ssize_t)self->store->size());
    if (!out) return nullptr;
    Py_ssize_t i = 0;
    bool bad = false;
    self->store->for_each([&](const std::string& k, CacheEntry& e) {
        if (bad) return;
        PyObject* t = Py_BuildValue("(NN)", key_py(k), entry_list(self, e));
        if (!t) {
            bad = true;
            return;
        }
        PyList_SET_ITEM(out, i++, t);
    });
    if (bad) {
        for (Py_ssize_t j = i; j < PyList_GET_SIZE(out); ++j) PyList_SET_ITEM(out, j, (Py_INCREF(Py_None), Py_None));
        Py_DECREF(out);
        return nullptr;
    }
    return out;
}

// to_records() -> [[uid, rv, phase, ns, name, core_text_or_None], ...] (checkpoint format)
PyObject* PodCache_to_records(PodCacheObject* self, PyObject*) {
    PyObject* out = PyList_New((Py_ssize_t)self->store->size());
    if (!out) return nullptr;
    Py_ssize_t i = 0;
    bool bad = false;
    self->store->for_each([&](const std::string& k, CacheEntry& e) {
        if (bad) return;
        PyObject* core = e.core ? PyUnicode_DecodeUTF8(e.core->data(), (Py_ssize_t)e.core->size(), "strict")
                                : (Py_INCREF(Py_None), Py_None);
        PyObject* r = Py_BuildValue("[NNNNNN]", key_py(k), opt_py(e.rv, e.rv_none),
                                    self->phases->py(e.phase_id), self->ns->py(e.ns_id),
                                    opt_py(e.name, e.name_none), core);
        if (!r) {
            bad = true;
            return;
        }
        PyList_SET_ITEM(out, i++, r);
    });
    if (bad) {
        for (Py_ssize_t j = i; j < PyList_GET_SIZE(out); ++j) PyList_SET_ITEM(out, j, (Py_INCREF(Py_None), Py_None));
        Py_DECREF(out);
        return nullptr;
    }
    return out;
}

PyObject* PodCache_load_records(PodCacheObject* self, PyObject* records) {
    PyObject* it = PyObject_GetIter(records);
    if (!it) return nullptr;
    PyObject* r;
    while ((r = PyIter_Next(it))) {
        PyObject *uid, *rv, *phase, *ns, *name, *core;
        PyObject* seq = PySequence_Fast(r, "checkpoint record must be a list");
        Py_DECREF(r);
        if (!seq) break;
        if (PySequence_Fast_GET_SIZE(seq) != 6) {
            Py_DECREF(seq);
            PyErr_SetString(PyExc_ValueError, "checkpoint record must have 6 fields");
            break;
        }
        PyObject** f = PySequence_Fast_ITEMS(seq);
        uid = f[0], rv = f[1], phase = f[2], ns = f[3], name = f[4], core = f[5];
        PyObject* cb = Py_None;
        Py_INCREF(cb);
        if (core != Py_None) {
            Py_DECREF(cb);
            cb = PyUnicode_AsUTF8String(core);
        }
        PyObject* res = cb ? PyObject_CallMethod((PyObject*)self, "put", "OOOOOO", uid, rv, phase, ns, name, cb)
                           : nullptr;
        Py_XDECREF(cb);
        Py_DECREF(seq);
        if (!res) break;
        Py_DECREF(res);
    }
    Py_DECREF(it);
    if (PyErr_Occurred()) return nullptr;
    Py_RETURN_NONE;
}

// memory() -> {"entries", "key_bytes", "core_bytes"}: what the cache holds (soak accounting)
PyObject* PodCache_memory(PodCacheObject* self, PyObject*) {
    size_t keys = 0, cores = 0;
    self->store->for_each([&](const std::string& k, CacheEntry& e) {
        keys += k.size() + e.rv.size() + e.name.size() + sizeof(CacheEntry) + 32;
        if (e.core) cores += e.core->size();
    });
    return Py_BuildValue("{snsnsn}", "entries", (Py_ssize_t)self->store->size(), "key_bytes", (Py_ssize_t)keys,
                         "core_bytes", (Py_ssize_t)cores);
}

// Namespace id of a (str | None) value: 0 for None; false when the text was
// never interned (then no entry can be in that namespace).
bool ns_lookup(PodCacheObject* self, PyObject* arg, uint32_t& id, bool& ok) {
    std::string s;
    bool none;
    ok = opt_text(arg, s, none);
    id = 0;
    if (!ok) return false;
    if (none) return true;
    auto it = self->ns->ids.find(std::string_view(s));
    if (it == self->ns->ids.end()) return false;
    id = it->second;
    return true;
}

// count_namespace(ns) -> pods cached in namespace ns (O(1): the per-namespace index)
PyObject* PodCache_count_namespace(PodCacheObject* self, PyObject* arg) {
    uint32_t id;
    bool ok;
    if (!ns_lookup(self, arg, id, ok)) {
        if (!ok) return nullptr;
        return PyLong_FromLong(0);
    }
    return PyLong_FromSsize_t((Py_ssize_t)self->store->count(id));
}

// Erase every entry of namespace id `ns`; returns how many.
size_t store_drop_namespace(PodStore& st, uint32_t ns) {
    size_t n = 0;
    while (CacheEntry* e = st.any_in(ns)) {
        st.erase(*e->key);
        ++n;
    }
    return n;
}

// Namespace ids named by an iterable of str | None, into `mark` (by id).
bool ns_marks(PodCacheObject* self, PyObject* names, std::vector<uint8_t>& mark) {
    mark.assign(self->store->ns_ids(), 0);
    PyObject* it = PyObject_GetIter(names);
    if (!it) return false;
    PyObject* item;
    while ((item = PyIter_Next(it))) {
        uint32_t id;
        bool ok;
        bool found = ns_lookup(self, item, id, ok);
        Py_DECREF(item);
        if (!ok) break;
        if (found && id < mark.size()) mark[id] = 1;
    }
    Py_DECREF(it);
    return !PyErr_Occurred();
}

// drop_namespaces(names) -> entries removed: forget (silently) every pod of
// those namespaces — a shard handing them over. Walks only their entries.
PyObject* PodCache_drop_namespaces(PodCacheObject* self, PyObject* names) {
    std::vector<uint8_t> mark;
    if (!ns_marks(self, names, mark)) return nullptr;
    size_t n = 0;
    for (uint32_t id = 0; id < mark.size(); ++id)
        if (mark[id]) n += store_drop_namespace(*self->store, id);
    return PyLong_FromSize_t(n);
}

// drop_namespaces_except(names) -> entries removed: every namespace not named.
PyObject* PodCache_drop_namespaces_except(PodCacheObject* self, PyObject* names) {
    std::vector<uint8_t> mark;
    if (!ns_marks(self, names, mark)) return nullptr;
    size_t n = 0;
    for (uint32_t id = 0; id < mark.size(); ++id)
        if (!mark[id]) n += store_drop_namespace(*self->store, id);
    return PyLong_FromSize_t(n);
}

// namespaces() -> {namespace: cached pods} for every namespace with at least one
PyObject* PodCache_namespaces(PodCacheObject* self, PyObject*) {
    PyObject* out = PyDict_New();
    if (!out) return nullptr;
    for (uint32_t id = 0; id < self->store->ns_ids(); ++id) {
        size_t n = self->store->count(id);
        if (!n) continue;
        PyObject* k = self->ns->py(id);
        PyObject* v = PyLong_FromSize_t(n);
        if (!k || !v || PyDict_SetItem(out, k, v) < 0) {
            Py_XDECREF(k);
            Py_XDECREF(v);
            Py_DECREF(out);
            return nullptr;
        }
        Py_DECREF(k);
        Py_DECREF(v);
    }
    return out;
}

PyObject* PodCache_clear(PodCacheObject* self, PyObject*) {
    self->store->clear();
    Py_RETURN_NONE;
}

// checkpoint.inc
PyObject* PodCache_snapshot(PodCacheObject* self, PyObject* args);
PyObject* PodCache_load_checkpoint(PodCacheObject* self, PyObject* args);

PyMethodDef PodCache_methods[] = {
    {"get", (PyCFunction)PodCache_get, METH_O, "get(uid) -> [rv, phase, ns, name, core] copy or None"},
    {"observe", (PyCFunction)PodCache_observe, METH_VARARGS,
     "observe(etype, uid, rv, phase, ns, name) -> previous phase or MISSING"},
    {"set_core", (PyCFunction)PodCache_set_core, METH_VARARGS, "set_core(uid, core)"},
    {"swap_failure", (PyCFunction)PodCache_swap_failure, METH_VARARGS,
     "swap_failure(uid, signature) -> previous failure signature (container failures)"},
    {"swap_condition", (PyCFunction)PodCache_swap_condition, METH_VARARGS,
     "swap_condition(uid, signature) -> previous condition signature (pod conditions)"},
    {"swap_terminating", (PyCFunction)PodCache_swap_terminating, METH_VARARGS,
     "swap_terminating(uid, signature) -> previous terminating signature (1 or 0)"},
    {"set_deadline", (PyCFunction)PodCache_set_deadline, METH_VARARGS,
     "set_deadline(uid, due | None): the pod's deletion deadline (None clears it and the reported mark)"},
    {"deadline", (PyCFunction)PodCache_deadline, METH_O, "deadline(uid) -> deletion deadline or None"},
    {"tracked", (PyCFunction)PodCache_tracked, METH_NOARGS, "tracked() -> entries with a deadline"},
    {"take_overdue", (PyCFunction)PodCache_take_overdue, METH_VARARGS,
     "take_overdue(now_s, after_s, scope_ns=None) -> [(uid, ns, name, core, deadline)]: overdue, unreported, marked now"},
    {"keep_core", (PyCFunction)PodCache_keep_core, METH_VARARGS,
     "keep_core(uid, core): the core of an unsent Pending line, dropped with the pending-since"},
    {"core_kept", (PyCFunction)PodCache_core_kept, METH_O, "core_kept(uid) -> whether the core is a kept one"},
    {"set_pending_since", (PyCFunction)PodCache_set_pending_since, METH_VARARGS,
     "set_pending_since(uid, since | None): creation time of a pod still Pending (None clears it, its mark, a kept core)"},
    {"pending_since", (PyCFunction)PodCache_pending_since, METH_O, "pending_since(uid) -> pending-since or None"},
    {"pending_tracked", (PyCFunction)PodCache_pending_tracked, METH_NOARGS,
     "pending_tracked() -> entries with a pending-since"},
    {"take_pending_overdue", (PyCFunction)PodCache_take_pending_overdue, METH_VARARGS,
     "take_pending_overdue(now_s, after_s, scope_ns=None) -> [(uid, ns, name, core, since)]: overdue, unreported, "
     "marked now"},
    {"put", (PyCFunction)PodCache_put, METH_VARARGS, "put(uid, rv, phase, ns, name, core=None)"},
    {"pop", (PyCFunction)PodCache_pop, METH_VARARGS, "pop(uid, default=None)"},
    {"items", (PyCFunction)PodCache_items, METH_NOARGS, "snapshot of (uid, entry) pairs"},
    {"to_records", (PyCFunction)PodCache_to_records, METH_NOARGS, "checkpoint records"},
    {"load_records", (PyCFunction)PodCache_load_records, METH_O, "add checkpoint records"},
    {"clear", (PyCFunction)PodCache_clear, METH_NOARGS, "drop every entry"},
    {"count_namespace", (PyCFunction)PodCache_count_namespace, METH_O, "count_namespace(ns) -> cached pods in ns"},
    {"drop_namespaces", (PyCFunction)PodCache_drop_namespaces, METH_O,
     "drop_namespaces(names) -> removed: forget every pod of these namespaces"},
    {"drop_namespaces_except", (PyCFunction)PodCache_drop_namespaces_except, METH_O,
     "drop_namespaces_except(names) -> removed: forget every pod outside these namespaces"},
    {"namespaces", (PyCFunction)PodCache_namespaces, METH_NOARGS, "{namespace: cached pods}"},
    {"memory", (PyCFunction)PodCache_memory, METH_NOARGS, "{entries, key_bytes, core_bytes}"},
    {"snapshot", (PyCFunction)PodCache_snapshot, METH_VARARGS,
     "snapshot(notifier=None) -> CacheSnapshot: entries + owed notifications, consistent (checkpoint.inc)"},
    {"load_checkpoint", (PyCFunction)PodCache_load_checkpoint, METH_VARARGS,
     "load_checkpoint(path) -> (header, owed): add a format-2 checkpoint's entries"},
    {nullptr, nullptr, 0, nullptr}};

PySequenceMethods PodCache_as_sequence = {};
PyTypeObject PodCacheType = {PyVarObject_HEAD_INIT(nullptr, 0)};

int register_podcache(PyObject* m) {
    PodCache_as_sequence.sq_length = (lenfunc)PodCache_len;
    PodCache_as_sequence.sq_contains = (objobjproc)PodCache_contains;
    PodCacheType.tp_name = "_kwcore.PodCache";
    PodCacheType.tp_basicsize = sizeof(PodCacheObject);
    PodCacheType.tp_flags = Py_TPFLAGS_DEFAULT;
    PodCacheType.tp_doc = "PodCache(missing=None): native uid -> [rv, phase, ns, name, core] cache";
    PodCacheType.tp_methods = PodCache_methods;
    PodCacheType.tp_as_sequence = &PodCache_as_sequence;
    PodCacheType.tp_new = PodCache_new;
    PodCacheType.tp_init = (initproc)PodCache_init;
    PodCacheType.tp_dealloc = (destructor)PodCache_dealloc;
    if (PyType_Ready(&PodCacheType) < 0) return -1;
    Py_INCREF(&PodCacheType);
    PyModule_AddObject(m, "PodCache", (PyObject*)&PodCacheType);
    return 0;
}
