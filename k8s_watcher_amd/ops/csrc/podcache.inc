// podcache.inc — native pod cache (_kwcore.PodCache). Unity-build fragment,
// #included into kwcore.cpp inside its anonymous namespace after podstore.inc
// and before engine.inc.
//
// Same contents and semantics as ops/cache.py's PodCache — one entry per live
// pod, uid -> [resourceVersion, phase, namespace, name, core] — but held in
// C++ (the PodStore of podstore.inc) so the fused Pipeline updates it without
// creating a Python object per event. The Python side (reconcile, checkpoint,
// tests) reaches it through the methods below, which convert on the way out.

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

// set_core(uid, core), and keep_core(uid, core) for kept: the payload core of
// an unsent Pending line (watcher.alerts.pending_overdue_seconds) or Running
// but unready one (unready_overdue_seconds), marked as kept, not sent:
// clearing that timer drops it, set_core replaces it.
// A pod not cached stores nothing.
PyObject* PodCache_store_core(PodCacheObject* self, PyObject* args, int kept) {
    PyObject* uid;
    Py_buffer core;
    if (!PyArg_ParseTuple(args, "Oy*", &uid, &core)) return nullptr;
    std::string k;
    bool ok = uid_key(uid, k);
    if (ok) {
        auto it = self->store->find(k);
        if (it != self->store->end()) {
            it->second.core = std::make_shared<const std::string>((const char*)core.buf, (size_t)core.len);
            it->second.core_kept = kept;
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

// The alert state, one implementation per verb: each takes the SigKind or
// TimerKind its name in the method table stands for (of_kind, below).

// swap_*(uid, signature) -> the pod's previous signature of that kind (0 for
// none, and for a pod not cached, which stores nothing); the kinds are independent
PyObject* PodCache_swap_sig(PodCacheObject* self, PyObject* args, int kind) {
    PyObject* uid;
    unsigned long long sig;
    if (!PyArg_ParseTuple(args, "OK", &uid, &sig)) return nullptr;
    std::string k;
    if (!uid_key(uid, k)) return nullptr;
    auto it = self->store->find(k);
    unsigned long long prev = 0;
    if (it != self->store->end()) {
        prev = it->second.sig[kind];
        it->second.sig[kind] = sig;
    }
    return PyLong_FromUnsignedLongLong(prev);
}

// set_deadline / set_pending_since / set_unready_since(uid, at | None): the
// pod's timer of that kind. None clears it and its reported mark (a kind that
// keeps cores: a kept core too), a value keeps the mark; an unknown uid is a no-op.
PyObject* PodCache_set_timer(PodCacheObject* self, PyObject* args, int kind) {
    PyObject *uid, *at;
    if (!PyArg_ParseTuple(args, "OO", &uid, &at)) return nullptr;
    std::string k;
    if (!uid_key(uid, k)) return nullptr;
    long long d = 0;
    if (at != Py_None) {
        d = PyLong_AsLongLong(at);
        if (d == -1 && PyErr_Occurred()) return nullptr;
    }
    auto it = self->store->find(k);
    if (it != self->store->end()) self->store->set_timer((TimerKind)kind, it, at != Py_None, (int64_t)d);
    Py_RETURN_NONE;
}

// deadline / pending_since(uid) -> the pod's timer of that kind or None
PyObject* PodCache_timer(PodCacheObject* self, PyObject* uid, int kind) {
    std::string k;
    if (!uid_key(uid, k)) return nullptr;
    auto it = self->store->find(k);
    if (it == self->store->end() || !it->second.timed[kind]) Py_RETURN_NONE;
    return PyLong_FromLongLong((long long)it->second.timer[kind].at);
}

// tracked / pending_tracked() -> entries with a timer of that kind
PyObject* PodCache_timed(PodCacheObject* self, PyObject*, int kind) {
    return PyLong_FromSize_t(self->store->timed((TimerKind)kind));
}

bool ns_lookup(PodCacheObject* self, PyObject* arg, uint32_t& id, bool& ok);

// take_overdue / take_pending_overdue(now_s, after_s, scope_ns=None)
//   -> [(uid, namespace, name, core, at), ...]: store_take_due of that kind
PyObject* PodCache_take_due(PodCacheObject* self, PyObject* args, int kind) {
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
    store_take_due(*self->store, (TimerKind)kind, now_s, after_s, scoped, ns_id, due);
    PyObject* out = PyList_New(0);
    if (!out) return nullptr;
    for (CacheEntry* e : due) {
        PyObject* t = Py_BuildValue("(NNNy#L)", key_py(*e->key), self->ns->py(e->ns_id), opt_py(e->name, e->name_none),
                                    e->core->data(), (Py_ssize_t)e->core->size(), (long long)e->timer[kind].at);
        if (!t || PyList_Append(out, t) < 0) {
            Py_XDECREF(t);
            Py_DECREF(out);
            return nullptr;
        }
        Py_DECREF(t);
    }
    return out;
}

// A method-table entry for one of the verbs above with its kind supplied.
template <PyObject* (*Verb)(PodCacheObject*, PyObject*, int), int Kind>
PyObject* of_kind(PodCacheObject* self, PyObject* arg) {
    return Verb(self, arg, Kind);
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
    {"set_core", (PyCFunction)of_kind<PodCache_store_core, false>, METH_VARARGS, "set_core(uid, core)"},
    {"swap_failure", (PyCFunction)of_kind<PodCache_swap_sig, SIG_FAIL>, METH_VARARGS,
     "swap_failure(uid, signature) -> previous failure signature (container failures)"},
    {"swap_condition", (PyCFunction)of_kind<PodCache_swap_sig, SIG_COND>, METH_VARARGS,
     "swap_condition(uid, signature) -> previous condition signature (pod conditions)"},
    {"swap_terminating", (PyCFunction)of_kind<PodCache_swap_sig, SIG_TERM>, METH_VARARGS,
     "swap_terminating(uid, signature) -> previous terminating signature (1 or 0)"},
    {"set_deadline", (PyCFunction)of_kind<PodCache_set_timer, TIMER_DEADLINE>, METH_VARARGS,
     "set_deadline(uid, due | None): the pod's deletion deadline (None clears it and the reported mark)"},
    {"deadline", (PyCFunction)of_kind<PodCache_timer, TIMER_DEADLINE>, METH_O,
     "deadline(uid) -> deletion deadline or None"},
    {"tracked", (PyCFunction)of_kind<PodCache_timed, TIMER_DEADLINE>, METH_NOARGS,
     "tracked() -> entries with a deadline"},
    {"take_overdue", (PyCFunction)of_kind<PodCache_take_due, TIMER_DEADLINE>, METH_VARARGS,
     "take_overdue(now_s, after_s, scope_ns=None) -> [(uid, ns, name, core, deadline)]: overdue, unreported, marked now"},
    {"keep_core", (PyCFunction)of_kind<PodCache_store_core, true>, METH_VARARGS,
     "keep_core(uid, core): the core of an unsent Pending line, dropped with the pending-since"},
    {"core_kept", (PyCFunction)PodCache_core_kept, METH_O, "core_kept(uid) -> whether the core is a kept one"},
    {"set_pending_since", (PyCFunction)of_kind<PodCache_set_timer, TIMER_PENDING>, METH_VARARGS,
     "set_pending_since(uid, since | None): creation time of a pod still Pending (None clears it, its mark, a kept core)"},
    {"pending_since", (PyCFunction)of_kind<PodCache_timer, TIMER_PENDING>, METH_O,
     "pending_since(uid) -> pending-since or None"},
    {"pending_tracked", (PyCFunction)of_kind<PodCache_timed, TIMER_PENDING>, METH_NOARGS,
     "pending_tracked() -> entries with a pending-since"},
    {"take_pending_overdue", (PyCFunction)of_kind<PodCache_take_due, TIMER_PENDING>, METH_VARARGS,
     "take_pending_overdue(now_s, after_s, scope_ns=None) -> [(uid, ns, name, core, since)]: overdue, unreported, "
     "marked now"},
    {"set_unready_since", (PyCFunction)of_kind<PodCache_set_timer, TIMER_UNREADY>, METH_VARARGS,
     "set_unready_since(uid, since | None): when a Running pod's Ready turned False (None clears it, its mark, a kept "
     "core)"},
    {"unready_since", (PyCFunction)of_kind<PodCache_timer, TIMER_UNREADY>, METH_O,
     "unready_since(uid) -> unready-since or None"},
    {"unready_tracked", (PyCFunction)of_kind<PodCache_timed, TIMER_UNREADY>, METH_NOARGS,
     "unready_tracked() -> entries with an unready-since"},
    {"take_unready_overdue", (PyCFunction)of_kind<PodCache_take_due, TIMER_UNREADY>, METH_VARARGS,
     "take_unready_overdue(now_s, after_s, scope_ns=None) -> [(uid, ns, name, core, since)]: overdue, unreported, "
     "marked now"},
    {"put",(PyCFunction)PodCache_put, METH_VARARGS, "put(uid, rv, phase, ns, name, core=None)"},
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
