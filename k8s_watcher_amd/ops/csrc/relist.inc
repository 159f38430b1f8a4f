// relist.inc — native LIST reconcile (_kwcore.Relist). Unity-build fragment,
// #included into kwcore.cpp after engine.inc (it drives a Pipeline).
//
// The reference has no recovery of its own: a second 410 raises out of
// kubernetes.watch, the process exits and the restart re-lists the whole
// cluster, replaying every pod as ADDED (/root/reference/watcher/
// pod_watcher.py:264,273-275; SURVEY §5.3 item 5). Here a 410 (or a restart
// without a usable checkpoint) LISTs the scope and diffs it against the pod
// cache: a new uid is ADDED, a changed resourceVersion MODIFIED, an unchanged
// one nothing, and a cached pod of the scope the LIST no longer has DELETED
// (payload from its cached core).
//
// Everything happens here, in bounded slices the event loop interleaves with
// the other scopes' watches:
//   * page(body): one LIST response (a PodList page). step() walks its items
//     array with the block scanner, fans the items out over the Pipeline's
//     DecodePool (the same decode as a watch line: field spans, critical
//     filter, payload core), compares each with the cache and feeds the
//     changed ones through the watch path's apply_line — filters, logs and
//     notifier exactly as for a watch event — until its time budget is spent.
//     No Python object per item, no copy of the cached cores.
//   * Every entry the LIST contains is stamped with this relist's generation;
//     sweep() then turns the scope's entries without it into DELETED. For a
//     namespace scope it walks only that namespace's list in the PodStore.
// Pages are applied as they arrive (a paginated LIST is one consistent
// snapshot), so no page outlives its step and nothing grows with the cluster
// but the cache itself.

uint32_t g_relist_gen = 0;  // loop thread only (GIL held)

uint32_t next_relist_gen() {
    if (++g_relist_gen == 0) ++g_relist_gen;  // 0 means "no relist"
    return g_relist_gen;
}

enum { RL_START, RL_ITEMS_FIRST, RL_ITEMS, RL_DONE };

constexpr size_t RELIST_BATCH = 128;  // items split, decoded and applied per round

// The most pods a LIST's metadata.remainingItemCount may make the cache
// reserve room for: 2^22, 28 times the 150,000 pods Kubernetes supports per
// cluster. A bucket is one pointer, so the hint costs at most 2^22 x 8 B =
// 32 MiB of bucket arrays over the whole store, whatever the server sends
// (tests/test_relist_sliced.py bounds a step's growth at 8 times that).
constexpr size_t RELIST_HINT_MAX = size_t(1) << 22;

struct RelistObject {
    PyObject_HEAD
    PipelineObject* pl;  // strong reference
    PyObject* body;      // current page (strong reference) or NULL
    Py_buffer view;
    const char* cur;
    const char* end;
    int state;
    std::string* page_rv;
    std::string* page_cont;
    bool have_rv, have_cont;
    uint32_t gen;
    bool silent;
    bool scoped;
    uint32_t scope_ns;
    std::vector<LineJob>* jobs;
    std::vector<std::string>* sweep_keys;
    size_t sweep_pos;
    bool sweep_ready;
    size_t sweep_bucket, sweep_nb;  // incremental walk of the hash table's buckets (sweep_collect)
    uint32_t sweep_shard;           // ... shard by shard (PodStore::SHARDS tables)
    // stats
    long long listed, added, modified, unchanged, deleted, invalid, pages, steps;
    int64_t busy_ns, max_step_ns;
};

void relist_release_page(RelistObject* self) {
    if (self->body) {
        PyBuffer_Release(&self->view);
        Py_CLEAR(self->body);
    }
    self->cur = self->end = nullptr;
}

PyObject* Relist_new(PyTypeObject* type, PyObject*, PyObject*) {
    RelistObject* self = (RelistObject*)type->tp_alloc(type, 0);
    if (!self) return nullptr;
    self->page_rv = new std::string();
    self->page_cont = new std::string();
    self->jobs = new std::vector<LineJob>();
    self->sweep_keys = new std::vector<std::string>();
    self->state = RL_DONE;
    return (PyObject*)self;
}

void Relist_dealloc(RelistObject* self) {
    relist_release_page(self);
    Py_XDECREF((PyObject*)self->pl);
    delete self->page_rv;
    delete self->page_cont;
    delete self->jobs;
    delete self->sweep_keys;
    Py_TYPE(self)->tp_free((PyObject*)self);
}

PyTypeObject RelistType = {PyVarObject_HEAD_INIT(nullptr, 0)};

// Pipeline.relist(scope_ns, notify) -> Relist
PyObject* Pipeline_relist(PipelineObject* self, PyObject* args) {
    PyObject* scope;
    int notify;
    if (!PyArg_ParseTuple(args, "Op", &scope, &notify)) return nullptr;
    std::string ns;
    bool none;
    if (!opt_text(scope, ns, none)) return nullptr;
    RelistObject* rl = (RelistObject*)Relist_new(&RelistType, nullptr, nullptr);
    if (!rl) return nullptr;
    Py_INCREF((PyObject*)self);
    rl->pl = self;
    rl->gen = next_relist_gen();
    rl->silent = !notify;
    rl->scoped = !none;
    rl->scope_ns = none ? 0 : self->cache->ns->intern(ns);
    return (PyObject*)rl;
}

// Relist.page(body): the next LIST response of this relist (kept until consumed)
PyObject* Relist_page(RelistObject* self, PyObject* arg) {
    if (self->body && self->state != RL_DONE) {
        PyErr_SetString(PyExc_RuntimeError, "Relist.page: the previous page is not consumed yet");
        return nullptr;
    }
    relist_release_page(self);
    if (PyObject_GetBuffer(arg, &self->view, PyBUF_SIMPLE) < 0) return nullptr;
    Py_INCREF(arg);
    self->body = arg;
    self->cur = (const char*)self->view.buf;
    self->end = self->cur + self->view.len;
    self->state = RL_START;
    self->have_rv = self->have_cont = false;
    self->page_rv->clear();
    self->page_cont->clear();
    ++self->pages;
    Py_RETURN_NONE;
}

// Relist.restart(): start the diff over (the LIST is being repeated from its
// first page); entries stamped by the earlier pages no longer count as seen.
PyObject* Relist_restart(RelistObject* self, PyObject*) {
    relist_release_page(self);
    self->state = RL_DONE;
    self->gen = next_relist_gen();
    self->sweep_keys->clear();
    self->sweep_pos = 0;
    self->sweep_ready = false;
    self->sweep_bucket = self->sweep_nb = 0;
    self->sweep_shard = 0;
    Py_RETURN_NONE;
}

// Advance the page's top-level state machine until the next item is found
// (returns true with its span) or the page ends (false, state RL_DONE).
// Throws ParseError on a malformed body.
bool relist_next_item(RelistObject* self, const char*& ip, size_t& in) {
    Parser P(self->cur, self->end);
    bool found = false;
    while (!found && self->state != RL_DONE) {
        switch (self->state) {
            case RL_START: {
                // The top level first, in one structural pass (the block scanner): a
                // repeated "items" or "metadata" key counts once, the last one, as
                // json.loads reads it; a "metadata" that is neither object nor null,
                // an "items" that is neither array nor null and trailing data fail
                // here, before any item is applied.
                Span items, md;
                P.object([&](const char* k, size_t kn) {
                    if (KEYIS("items")) items = P.value();
                    else if (KEYIS("metadata")) md = P.value();
                    else P.value();
                });
                P.ws();
                if (P.p_ != P.end_) P.fail("trailing data");
                if (md.present() && !md.is_null()) {
                    if (md.p[0] != '{') P.fail("metadata is not an object");
                    Parser M(md.p, md.p + md.n);
                    M.object([&](const char* k, size_t kn) {
                        Span v = M.value();
                        if (KEYIS("resourceVersion")) {  // (a repeated key: the last one counts)
                            if ((self->have_rv = v.is_string())) *self->page_rv = span_text(v);
                        } else if (KEYIS("continue")) {
                            if ((self->have_cont = v.is_string() && v.n > 2)) *self->page_cont = span_text(v);
                        } else if (KEYIS("remainingItemCount") && v.n && v.n < 12 && is_digit(v.p[0])) {
                            // the pods still to come: grow the cache's hash table for them
                            // now, while it is small, rather than rehash 100k entries
                            // mid-relist (~20 ms in one slice). The number is the server's
                            // and only an optimisation: clamped, and a reservation that
                            // fails is skipped (the tables then grow as the items arrive).
                            const size_t more = std::min<size_t>(
                                (size_t)std::strtoull(std::string(v.p, v.n).c_str(), nullptr, 10), RELIST_HINT_MAX);
                            PodStore& st = *self->pl->cache->store;
                            try {
                                st.reserve(more + RELIST_BATCH * 4);
                            } catch (const std::bad_alloc&) {
                            } catch (const std::length_error&) {
                            }
                        }
                    });
                }
                if (!items.present() || items.is_null()) {
                    self->state = RL_DONE;
                } else {
                    if (items.p[0] != '[') P.fail("items is not an array");
                    P.p_ = items.p + 1;
                    self->state = RL_ITEMS_FIRST;
                }
                break;
            }
            case RL_ITEMS_FIRST:
                if (P.peek() == ']') {
                    ++P.p_;
                    self->state = RL_DONE;  // (RL_START saw the rest of the body)
                } else {
                    self->state = RL_ITEMS;
                }
                break;
            case RL_ITEMS: {
                const bool obj = P.peek() == '{';
                Span v = P.value();  // the block scanner: bracket-matched, strings skipped
                char c = P.peek();
                ++P.p_;
                if (c == ']') self->state = RL_DONE; else if (c != ',') P.fail("expected , or ]");
                if (obj) {  // anything else in items is ignored, as decode_list does
                    ip = v.p;
                    in = v.n;
                    found = true;
                }
                break;
            }
        }
    }
    self->cur = P.p_;
    return found;
}

// Pass 1 done (fields only): compare one LIST item with the cache (GIL held,
// list order). An unchanged resourceVersion only marks the entry seen; a
// changed or new pod gets its event type and goes to the payload pass.
void relist_classify(RelistObject* self, LineJob& J) {
    ++self->listed;
    if (J.err) {
        J.stage = JOB_SKIP;  // reported as INVALID at apply time
        return;
    }
    const PodSpans& S = J.S;
    std::string kbuf;
    std::string_view key = NONE_UID;
    if (S.uid.is_string() && !span_view(S.uid, key)) {
        kbuf = span_text(S.uid);
        key = kbuf;
    }
    PodStore& store = *self->pl->cache->store;
    auto it = store.find(key);
    if (it != store.end()) {
        CacheEntry& e = it->second;
        bool same;
        if (!S.rv.is_string()) {
            same = e.rv_none;
        } else {
            std::string_view rv;
            if (span_view(S.rv, rv)) {
                same = !e.rv_none && e.rv == rv;
            } else {
                same = !e.rv_none && e.rv == span_text(S.rv);
            }
        }
        if (same) {
            // a notifying relist stores the deadline of an unchanged pod too: a
            // cache rebuilt from a checkpoint or a hand-over has the entry and
            // no deadline (the light parse kept the span)
            if (self->pl->deadlines && !self->silent) {
                int64_t due = 0;
                const bool has = deletion_deadline(S, due);
                if (has || e.timed[TIMER_DEADLINE]) store.set_timer(TIMER_DEADLINE, it, has, due);
            }
            // ... and its pending-since, likewise (watcher.alerts.pending_overdue_seconds)
            if (__builtin_expect(self->pl->pending, 0) && !self->silent) {
                int64_t since = 0;
                const bool has = pending_since(S, since);
                if (has || e.timed[TIMER_PENDING]) store.set_timer(TIMER_PENDING, it, has, since);
            }
            // ... and its unready-since (watcher.alerts.unready_overdue_seconds; the
            // light parse kept the conditions span, walked for a Running pod only)
            if (__builtin_expect(self->pl->unready, 0) && !self->silent) {
                int64_t since = 0;
                const bool has = unready_since(S, since);
                if (has || e.timed[TIMER_UNREADY]) store.set_timer(TIMER_UNREADY, it, has, since);
            }
            e.list_gen = self->gen;
            ++self->unchanged;
            J.stage = JOB_SKIP;
            J.tidx = -3;
            return;
        }
        J.tidx = T_MODIFIED;
        ++self->modified;
    } else {
        J.tidx = T_ADDED;
        ++self->added;
    }
    J.stage = self->silent ? JOB_SKIP : JOB_PAYLOAD;  // a silent relist never needs the payload
}

// Pass 2 done: the item through the watch path (cache, filters, notify).
void relist_apply_item(RelistObject* self, LineJob& J) {
    PipelineObject* pl = self->pl;
    if (J.err) {
        ++self->invalid;
        pl_ctrl(pl, make_invalid(J.err, J.p, J.n));
        return;
    }
    if (J.tidx == -3) return;  // unchanged
    apply_line(pl, J);
}

// Per-call state of the pipeline (as pl_run sets it up) around a relist slice.
void relist_call_begin(RelistObject* self, int64_t read_ns) {
    PipelineObject* pl = self->pl;
    pl->ctrl = PyList_New(0);
    pl->logs = nullptr;
    pl->submits = nullptr;
    pl->have_rv = false;
    pl->rv_span = Span();
    pl->ts->clear();
    pl->c_recv = pl->c_crit = pl->c_ns = pl->c_unch = pl->c_shard = pl->c_bm = pl->c_fail = pl->c_cond = pl->c_term = 0;
    pl->read_ns = read_ns;
    pl->failed = pl->ctrl == nullptr;
    pl->relist_gen = self->gen;
    pl->silent = self->silent;
}

// -> (done, ctrl, logs, submits) or NULL with the error set
PyObject* relist_call_end(RelistObject* self, bool done, int64_t t0) {
    PipelineObject* pl = self->pl;
    pl->relist_gen = 0;
    pl->silent = false;
    const int64_t dt = mono_ns() - t0;
    self->busy_ns += dt;
    if (dt > self->max_step_ns) self->max_step_ns = dt;
    ++self->steps;
    PyObject* m = pl->metrics;
    counter_add(m, "events_received", pl->c_recv);
    counter_add(m, "events_filtered_critical", pl->c_crit);
    counter_add(m, "events_filtered_namespace", pl->c_ns);
    counter_add(m, "events_unchanged", pl->c_unch);
    counter_add(m, "events_other_shard", pl->c_shard);
    counter_add(m, "events_container_failure", pl->c_fail);
    counter_add(m, "events_pod_condition", pl->c_cond);
    counter_add(m, "events_terminating", pl->c_term);
    if (pl->failed || PyErr_Occurred()) {
        Py_CLEAR(pl->ctrl);
        Py_CLEAR(pl->logs);
        Py_CLEAR(pl->submits);
        if (!PyErr_Occurred()) PyErr_SetString(PyExc_RuntimeError, "native relist failure");
        return nullptr;
    }
    PyObject* logs = pl->logs ? pl->logs : (Py_INCREF(Py_None), Py_None);
    PyObject* subs = pl->submits ? pl->submits : (Py_INCREF(Py_None), Py_None);
    PyObject* res = Py_BuildValue("(ONNN)", done ? Py_True : Py_False, pl->ctrl, logs, subs);
    pl->ctrl = pl->logs = pl->submits = nullptr;
    return res;
}

bool parse_budget(PyObject* args, int64_t& budget_ns, long long& read_ns) {
    double budget_us;
    if (!PyArg_ParseTuple(args, "dL", &budget_us, &read_ns)) return false;
    budget_ns = budget_us <= 0 ? 0 : (int64_t)(budget_us * 1000.0);
    return true;
}

// Relist.step(budget_us, read_ns) -> (done, ctrl, logs, submits): apply the
// current page's items until the page ends (done) or budget_us has passed.
PyObject* Relist_step(RelistObject* self, PyObject* args) {
    int64_t budget;
    long long read_ns;
    if (!parse_budget(args, budget, read_ns)) return nullptr;
    if (!self->body) {
        PyErr_SetString(PyExc_RuntimeError, "Relist.step: no page");
        return nullptr;
    }
    const int64_t t0 = mono_ns();
    relist_call_begin(self, read_ns);
    PipelineObject* pl = self->pl;
    std::vector<LineJob>& jobs = *self->jobs;
    // items are always parsed filter-first: most of a relist is unchanged pods,
    // whose spec and status arrays are never walked
    DecodeCfg cfg = *pl->cfg;
    cfg.light = true;
    DecodePool* pool = pl->pool;
    const char* perr = nullptr;
    PayloadTally payloads;
    while (!pl->failed && self->state != RL_DONE) {
        size_t nj = 0;
        try {
            const char* ip;
            size_t in;
            while (nj < RELIST_BATCH && relist_next_item(self, ip, in)) {
                if (nj == jobs.size()) jobs.emplace_back();
                LineJob& J = jobs[nj++];
                J.p = ip;
                J.n = in;
                J.bare = true;
                J.stage = JOB_FIELDS;
                J.read_ns = pl->read_ns;
            }
        } catch (const ParseError& e) {
            perr = e.msg;  // the items found before the error are still applied
            self->state = RL_DONE;
        }
        // pass 1: fields of every item (parallel), then the cache comparison (here, in order)
        const bool par1 = pool && nj >= PARALLEL_MIN_LINES;
        if (par1) {
            pool->start(jobs.data(), (uint32_t)nj, &cfg);
            pool->finish((uint32_t)nj);
        }
        size_t changed = 0;
        for (size_t i = 0; i < nj; ++i) {
            if (!par1) decode_line(cfg, jobs[i]);
            relist_classify(self, jobs[i]);
            changed += jobs[i].stage == JOB_PAYLOAD;
        }
        // pass 2: payloads of the changed ones (parallel) while this thread applies in order
        // (decode_payload: a changed item of a namespace the filter drops, or
        // of another shard, gets no payload — the watch path's pre-filter)
        if (pool && changed >= PARALLEL_MIN_LINES) {
            pool->start(jobs.data(), (uint32_t)nj, &cfg);
            for (size_t i = 0; i < nj && !pl->failed; ++i) {
                pool->await((uint32_t)i);
                payloads.see(jobs[i].hot);
                relist_apply_item(self, jobs[i]);
                pl_pump(pl, i);
            }
            pool->finish((uint32_t)nj);
        } else {
            for (size_t i = 0; i < nj && !pl->failed; ++i) {
                decode_line(cfg, jobs[i]);
                payloads.see(jobs[i].hot);
                relist_apply_item(self, jobs[i]);
                pl_pump(pl, i);
            }
        }
        payloads.flush();
        if (mono_ns() - t0 >= budget) break;
    }
    const bool done = self->state == RL_DONE;
    if (done) relist_release_page(self);
    if (perr && !pl->failed) {
        pl->failed = true;
        PyErr_Format(PyExc_ValueError, "invalid list body: %s", perr);
    }
    return relist_call_end(self, done, t0);
}

// Relist.page_meta() -> (resourceVersion | None, continue | None) of the last page
PyObject* Relist_page_meta(RelistObject* self, PyObject*) {
    PyObject* rv = self->have_rv ? PyUnicode_DecodeUTF8(self->page_rv->data(), (Py_ssize_t)self->page_rv->size(),
                                                        "replace")
                                 : (Py_INCREF(Py_None), Py_None);
    PyObject* co = self->have_cont ? PyUnicode_DecodeUTF8(self->page_cont->data(),
                                                          (Py_ssize_t)self->page_cont->size(), "replace")
                                   : (Py_INCREF(Py_None), Py_None);
    return Py_BuildValue("(NN)", rv, co);
}

// The payload core of a pod known only from the cache (never notified):
// decoder.core_from_summary's bytes (uid, namespace, name, phase; no status
// but the phase, no spec).
void summary_core(std::string& o, PipelineObject* pl, std::string_view uid, bool uid_none, uint32_t ns_id,
                  const std::string& name, bool name_none, uint32_t phase_id) {
    std::string u, n, m, p;
    PodSpans S;
    S.meta_present = true;
    auto quoted = [](std::string& dst, std::string_view text, bool none) {
        if (none) dst = "null"; else json_quote(dst, text);
        return Span{dst.data(), dst.size()};
    };
    S.uid = quoted(u, uid, uid_none);
    S.ns = quoted(n, pl->cache->ns->text[ns_id], ns_id == 0);
    S.name = quoted(m, name, name_none);
    if (phase_id) {
        S.status_present = true;
        S.phase = quoted(p, pl->cache->phases->text[phase_id], false);
    }
    build_core(o, S, *pl->env_json, pl->cfg->extra);
}

// DELETED for a cached pod the LIST did not contain (GIL held).
void relist_delete(RelistObject* self, PodStore::iterator it) {
    PipelineObject* pl = self->pl;
    PodCacheObject* cache = pl->cache;
    const std::string uid = it->first;
    const bool uid_none = uid == NONE_UID;
    CacheEntry& e = it->second;
    const uint32_t ns_id = e.ns_id, phase_id = e.phase_id;
    const std::string& ns_text = cache->ns->text[ns_id];
    if (pl->shard_count > 1) {  // as the watch path: the other shard's business
        const std::string& k = pl->shard_by_uid ? uid : ns_text;
        const std::string_view kv = (pl->shard_by_uid && uid_none) ? std::string_view() : std::string_view(k);
        if ((int)(crc32_bytes(kv.data(), kv.size()) % (uint32_t)pl->shard_count) != pl->shard_index) {
            ++pl->c_shard;
            return;
        }
    }
    const std::string name = e.name;
    const bool name_none = e.name_none;
    CoreRef core = e.core;
    cache->store->erase(it);
    if (pl->silent) return;
    ++pl->c_recv;
    ++self->deleted;
    const bool ns_str = ns_id != 0;
    if (pl->log_events) {  // pod_watcher.py:223
        if (pl->sink) {
            LogSink& L = *pl->sink->sink;
            std::lock_guard<std::mutex> g(L.mu);
            L.begin(20);
            L.add("Pod event detected: DELETED - ");
            if (ns_str) L.add(ns_text); else L.add("None", 4);
            L.add("/", 1);
            if (!name_none) L.add(name); else L.add("None", 4);
            L.end();
        } else {
            std::string msg = "Pod event detected: DELETED - " + (ns_str ? ns_text : std::string("None")) + "/" +
                              (name_none ? std::string("None") : name);
            pl_log(pl, 20, PyUnicode_DecodeUTF8(msg.data(), (Py_ssize_t)msg.size(), "replace"));
        }
    }
    if (pl->nsset) {
        const std::vector<uint8_t>& allowed = *pl->ns_allowed;
        if (!(ns_id < allowed.size() && allowed[ns_id])) {
            if (pl->log_debug) {  // pod_watcher.py:228
                std::string msg = "Skipping pod " + (ns_str ? ns_text : std::string("None")) + "/" +
                                  (name_none ? std::string("None") : name) + " - not in target namespaces";
                if (pl->sink) {
                    LogSink& L = *pl->sink->sink;
                    std::lock_guard<std::mutex> g(L.mu);
                    L.begin(10);
                    L.add(msg);
                    L.end();
                } else {
                    pl_log(pl, 10, PyUnicode_DecodeUTF8(msg.data(), (Py_ssize_t)msg.size(), "replace"));
                }
            }
            ++pl->c_ns;
            return;
        }
    }
    std::string body;
    if (core) body.assign(*core); else summary_core(body, pl, uid, uid_none, ns_id, name, name_none, phase_id);
    event_ts(*pl->ts, pl->ts_utc);
    if (pl->notifier) {
        body.pop_back();
        body.append(",\"event_timestamp\":\"");
        body.append(*pl->ts);
        body.append("\",\"event_type\":\"DELETED\"}");
        std::lock_guard<std::recursive_mutex> g(pl->notifier->core->mu);
        pl->notifier->core->submit(uid_none ? std::string_view("None") : std::string_view(uid), "DELETED",
                                   ns_str ? std::string_view(ns_text) : std::string_view("None"),
                                   name_none ? std::string_view("None") : std::string_view(name), body,
                                   std::string_view(), pl->read_ns);
        return;
    }
    auto str_or_none = [](const std::string& s, bool none) -> PyObject* {
        if (none) Py_RETURN_NONE;
        return PyUnicode_DecodeUTF8(s.data(), (Py_ssize_t)s.size(), "replace");
    };
    PyObject* uo = str_or_none(uid, uid_none);
    PyObject* nso = str_or_none(ns_text, !ns_str);
    PyObject* nmo = str_or_none(name, name_none);
    PyObject* co = PyBytes_FromStringAndSize(body.data(), (Py_ssize_t)body.size());
    PyObject* tso = PyUnicode_FromStringAndSize(pl->ts->data(), (Py_ssize_t)pl->ts->size());
    PyObject* t = (uo && nso && nmo && co && tso) ? PyTuple_Pack(6, uo, g_types[T_DELETED], nso, nmo, co, tso)
                                                  : nullptr;
    Py_XDECREF(uo);
    Py_XDECREF(nso);
    Py_XDECREF(nmo);
    Py_XDECREF(co);
    Py_XDECREF(tso);
    if (!pl->submits && t) pl->submits = PyList_New(0);
    if (!t || !pl->submits || PyList_Append(pl->submits, t) < 0) pl->failed = true;
    Py_XDECREF(t);
}

// The uids of the scope's entries this relist did not see (later slices look
// each up again). A namespace's own list when it is short; otherwise the hash
// table bucket by bucket, resumable across slices: walking 100k scattered
// nodes is ~20 ms of cache misses. A rehash between slices restarts the walk
// (a key taken twice is harmless: the second lookup finds it gone).
bool sweep_collect(RelistObject* self, int64_t t0, int64_t budget) {
    PodStore& store = *self->pl->cache->store;
    std::vector<std::string>& keys = *self->sweep_keys;
    if (self->scoped && store.count(self->scope_ns) <= 4096) {
        store.for_each_in(self->scope_ns, [&](CacheEntry& e) {
            if (e.list_gen != self->gen) keys.push_back(*e.key);
        });
        self->sweep_ready = true;
        return true;
    }
    bool out_of_time = false;
    while (!out_of_time && self->sweep_shard < PodStore::SHARDS) {
        auto& m = store.shard_map(self->sweep_shard);
        if (m.bucket_count() != self->sweep_nb) {  // a new shard, or this one rehashed since the last slice
            self->sweep_nb = m.bucket_count();
            self->sweep_bucket = 0;
        }
        size_t b = self->sweep_bucket;
        for (; b < self->sweep_nb; ++b) {
            for (auto it = m.begin(b); it != m.end(b); ++it)
                if (it->second.list_gen != self->gen && (!self->scoped || it->second.ns_id == self->scope_ns))
                    keys.push_back(it->first);
            if ((b & 1023) == 1023 && mono_ns() - t0 >= budget) {
                ++b;
                out_of_time = true;
                break;
            }
        }
        self->sweep_bucket = b;
        if (b >= self->sweep_nb) {
            ++self->sweep_shard;
            self->sweep_nb = 0;
        }
    }
    self->sweep_ready = self->sweep_shard >= PodStore::SHARDS;
    return self->sweep_ready;
}

// Relist.sweep(budget_us, read_ns) -> (done, ctrl, logs, submits): DELETED for
// every cached pod of the scope the LIST did not contain, in slices.
PyObject* Relist_sweep(RelistObject* self, PyObject* args) {
    int64_t budget;
    long long read_ns;
    if (!parse_budget(args, budget, read_ns)) return nullptr;
    const int64_t t0 = mono_ns();
    PodStore& store = *self->pl->cache->store;
    if (!self->sweep_ready && !sweep_collect(self, t0, budget)) {  // still walking the table
        relist_call_begin(self, read_ns);
        return relist_call_end(self, false, t0);
    }
    relist_call_begin(self, read_ns);
    PipelineObject* pl = self->pl;
    std::vector<std::string>& keys = *self->sweep_keys;
    size_t i = self->sweep_pos;
    for (size_t n = 0; i < keys.size() && !pl->failed; ++i, ++n) {
        auto it = store.find(keys[i]);
        if (it != store.end() && it->second.list_gen != self->gen) relist_delete(self, it);
        if ((n & 63) == 63) {
            pl_pump(pl, PUMP_LINES - 1);
            if (mono_ns() - t0 >= budget) {
                ++i;
                break;
            }
        }
    }
    self->sweep_pos = i;
    const bool done = i >= keys.size();
    if (done) {
        keys.clear();
        keys.shrink_to_fit();
    }
    return relist_call_end(self, done, t0);
}

// ----------------------------------------------------------------------------- overdue sweep
//
// Pipeline.report_overdue(now_s, after_s, scope_ns, read_ns, pending=False, kind=None)
//   -> (sent, ctrl, logs, submits)
// watcher.alerts.terminating_overdue_seconds, pending_overdue_seconds and
// unready_overdue_seconds: the sends no watch line causes. kind is the
// TimerKind swept (0 deadline, 1 pending, 2 unready); without it, pending
// true picks 1 and false 0, as before there was a third. Every cached pod (of
// namespace scope_ns, or any for None) that at now_s is after_s or more past
// its timer of that kind (its deletion deadline, its creation time while still
// Pending, the time its Ready turned False while Running), was not reported yet
// and has a payload core is marked and notified as MODIFIED: the cached core
// with an "alert" member spliced in before its closing brace (the cache keeps
// the core as it was), keyed by uid like any event, so a DELETED that follows
// stays behind it. The kinds differ in the timer (its list and mark) and
// in their row of k_sweep_text; everything else is one code path. Walks the
// timed lists only and erases nothing: it runs on the loop thread outside a
// batch, also between two slices of a relist on the same cache. Log lines and
// (asyncio pool) submissions come back as a relist slice's do.

// What a sweep of each TimerKind says (engine/pipeline.py _SweepKind is its twin).
struct SweepText {
    const char *log_head, *log_tail, *alert_head, *alert_mid, *counter;
};
const SweepText k_sweep_text[N_TIMER] = {
    {"Pod termination overdue: ", "s past deletionTimestamp",
     ",\"alert\":{\"kind\":\"termination_overdue\",\"deadline_unix\":", ",\"overdue_seconds\":",
     "events_termination_overdue"},
    {"Pod pending overdue: ", "s since creationTimestamp",
     ",\"alert\":{\"kind\":\"pending_overdue\",\"since_unix\":", ",\"pending_seconds\":",
     "events_pending_overdue"},
    {"Pod unready overdue: ", "s since Ready=False",
     ",\"alert\":{\"kind\":\"unready_overdue\",\"since_unix\":", ",\"unready_seconds\":",
     "events_unready_overdue"},
};
PyObject* Pipeline_report_overdue(PipelineObject* pl, PyObject* args, PyObject* kwargs) {
    long long now_s, after_s, read_ns;
    PyObject *scope, *which = Py_None;
    int pending = 0;
    static const char* kwlist[] = {"now_s", "after_s", "scope_ns", "read_ns", "pending", "kind", nullptr};
    if (!PyArg_ParseTupleAndKeywords(args, kwargs, "LLOL|pO", (char**)kwlist, &now_s, &after_s, &scope, &read_ns,
                                     &pending, &which))
        return nullptr;
    TimerKind kind = pending ? TIMER_PENDING : TIMER_DEADLINE;
    if (which != Py_None) {
        const long k = PyLong_AsLong(which);
        if (k == -1 && PyErr_Occurred()) return nullptr;
        if (k < 0 || k >= N_TIMER) {
            PyErr_SetString(PyExc_ValueError, "report_overdue: no such kind");
            return nullptr;
        }
        kind = (TimerKind)k;
    }
    const SweepText& text = k_sweep_text[kind];
    if (pl->ctrl) {
        PyErr_SetString(PyExc_RuntimeError, "report_overdue: inside a batch");
        return nullptr;
    }
    PodCacheObject* cache = pl->cache;
    uint32_t scope_ns = 0;
    bool known = true;
    if (scope != Py_None) {
        bool ok;
        known = ns_lookup(cache, scope, scope_ns, ok);
        if (!ok) return nullptr;
    }
    std::vector<CacheEntry*> due;
    if (known) store_take_due(*cache->store, kind, now_s, after_s, scope != Py_None, scope_ns, due);
    pl->ctrl = PyList_New(0);
    if (!pl->ctrl) return nullptr;
    pl->logs = pl->submits = nullptr;
    pl->ts->clear();
    pl->read_ns = read_ns;
    pl->failed = false;
    const std::string none("None");
    std::string body, msg;
    long long sent = 0;
    for (CacheEntry* e : due) {
        if (pl->failed) break;
        const bool uid_none = *e->key == NONE_UID;
        const std::string& uid = uid_none ? none : *e->key;
        const std::string& ns_text = e->ns_id ? cache->ns->text[e->ns_id] : none;
        const std::string& name = e->name_none ? none : e->name;
        const long long at = (long long)e->timer[kind].at;
        const long long late = (long long)((__int128)now_s - (__int128)at);
        if (pl->log_events) {
            msg.assign(text.log_head).append(ns_text).append("/").append(name).append(" - ");
            msg.append(std::to_string(late)).append(text.log_tail);
            if (pl->sink) {
                LogSink& L = *pl->sink->sink;
                std::lock_guard<std::mutex> g(L.mu);
                L.begin(20);
                L.add(msg);
                L.end();
            } else {
                pl_log(pl, 20, PyUnicode_DecodeUTF8(msg.data(), (Py_ssize_t)msg.size(), "replace"));
            }
        }
        body.assign(*e->core);
        body.pop_back();
        body.append(text.alert_head);
        body.append(std::to_string(at));
        body.append(text.alert_mid);
        body.append(std::to_string(late));
        body.append("}}");
        event_ts(*pl->ts, pl->ts_utc);
        ++sent;
        if (pl->notifier) {
            body.pop_back();
            append_body_tail(body, *pl->ts, "MODIFIED");
            std::lock_guard<std::recursive_mutex> g(pl->notifier->core->mu);
            pl->notifier->core->submit(uid, "MODIFIED", ns_text, name, body, std::string_view(), pl->read_ns);
            continue;
        }
        PyObject* uo = uid_none ? (Py_INCREF(Py_None), Py_None) : key_py(uid);
        PyObject* nso = cache->ns->py(e->ns_id);
        PyObject* nmo = opt_py(e->name, e->name_none);
        PyObject* co = PyBytes_FromStringAndSize(body.data(), (Py_ssize_t)body.size());
        PyObject* tso = PyUnicode_FromStringAndSize(pl->ts->data(), (Py_ssize_t)pl->ts->size());
        PyObject* t = (uo && nso && nmo && co && tso) ? PyTuple_Pack(6, uo, g_types[T_MODIFIED], nso, nmo, co, tso)
                                                      : nullptr;
        Py_XDECREF(uo);
        Py_XDECREF(nso);
        Py_XDECREF(nmo);
        Py_XDECREF(co);
        Py_XDECREF(tso);
        if (!pl->submits && t) pl->submits = PyList_New(0);
        if (!t || !pl->submits || PyList_Append(pl->submits, t) < 0) pl->failed = true;
        Py_XDECREF(t);
    }
    counter_add(pl->metrics, text.counter, sent);
    if (pl->failed || PyErr_Occurred()) {
        Py_CLEAR(pl->ctrl);
        Py_CLEAR(pl->logs);
        Py_CLEAR(pl->submits);
        if (!PyErr_Occurred()) PyErr_SetString(PyExc_RuntimeError, "native overdue sweep failure");
        return nullptr;
    }
    PyObject* logs = pl->logs ? pl->logs : (Py_INCREF(Py_None), Py_None);
    PyObject* subs = pl->submits ? pl->submits : (Py_INCREF(Py_None), Py_None);
    PyObject* res = Py_BuildValue("(LNNN)", sent, pl->ctrl, logs, subs);
    pl->ctrl = pl->logs = pl->submits = nullptr;
    return res;
}

PyObject* Relist_stats(RelistObject* self, PyObject*) {
    return Py_BuildValue("{s:L,s:L,s:L,s:L,s:L,s:L,s:L,s:L,s:d,s:d}", "listed", self->listed, "added", self->added,
                         "modified", self->modified, "unchanged", self->unchanged, "deleted", self->deleted,
                         "invalid", self->invalid, "pages", self->pages, "steps", self->steps, "busy_s",
                         (double)self->busy_ns * 1e-9, "max_step_s", (double)self->max_step_ns * 1e-9);
}

PyMethodDef Relist_methods[] = {
    {"page", (PyCFunction)Relist_page, METH_O, "page(body): the next LIST response to apply"},
    {"step", (PyCFunction)Relist_step, METH_VARARGS,
     "step(budget_us, read_ns) -> (done, ctrl, logs, submits): apply the page's items for up to budget_us"},
    {"page_meta", (PyCFunction)Relist_page_meta, METH_NOARGS, "(resourceVersion, continue) of the last page"},
    {"restart", (PyCFunction)Relist_restart, METH_NOARGS, "the LIST starts over: earlier pages no longer count"},
    {"sweep", (PyCFunction)Relist_sweep, METH_VARARGS,
     "sweep(budget_us, read_ns) -> (done, ctrl, logs, submits): DELETED for the scope's pods the LIST lacked"},
    {"stats", (PyCFunction)Relist_stats, METH_NOARGS, "items listed/added/modified/unchanged/deleted, time"},
    {nullptr, nullptr, 0, nullptr}};

// ============================================================================= WatchList collector
//
// _kwcore.WatchList(): the initial state of a WatchList watch
// (sendInitialEvents=true, KEP-3157) fed into a native Relist instead of a
// Python dict (VERDICT round 3, item 5). feed(data, framed) de-chunks and
// splits the stream and turns it into segments, in stream order:
//   (0, page)   ADDED / MODIFIED objects of this read as a PodList page body,
//               for Relist.page — compared with the cache like LIST items
//               (a MODIFIED of a pod seen earlier in the stream is simply its
//               newer state), stamped with the relist's generation
//   (1, line)   a DELETED event line, for the Pipeline's watch path (the pod
//               leaves the cache and is notified, as a watch would do)
//   (2, status) an ERROR event's object (410: relist)
//   (3, rv)     the initial-events-end bookmark: its resourceVersion; the
//               caller sweeps (Relist.sweep) and resumes watching from it
//   (4, reason) a line that is not a watch event (reported, skipped)
// Nothing is kept past a feed() but a partial line: the state is applied as
// it arrives, read by read, like LIST pages.

struct WatchListObject {
    PyObject_HEAD
    std::string* partial;     // a line continuing in the next read
    ChunkState chunk;         // feed(data, True)'s framing state (chunked.inc)
    bool done;
    long long lines, items, deleted, invalid, bytes;
};

PyObject* WatchList_new(PyTypeObject* type, PyObject*, PyObject*) {
    WatchListObject* self = (WatchListObject*)type->tp_alloc(type, 0);
    if (!self) return nullptr;
    self->partial = new std::string();
    new (&self->chunk) ChunkState();
    return (PyObject*)self;
}

void WatchList_dealloc(WatchListObject* self) {
    delete self->partial;
    self->chunk.~ChunkState();
    Py_TYPE(self)->tp_free((PyObject*)self);
}

struct WlOut {
    PyObject* segs;
    std::string page;  // items of the page being built, comma-separated
    size_t page_items = 0;
    // uids in `page`: a Relist page is classified against the cache as a
    // whole before any item applies, so a uid seen twice (a server streaming
    // live events before the end bookmark) closes the page and starts a new
    // one — its second object is then compared with the first, not with the
    // cache state before both (ADDED then MODIFIED, not ADDED twice)
    std::unordered_set<std::string> page_uids;
    bool failed = false;
    void add(int kind, PyObject* payload) {
        PyObject* t = payload ? Py_BuildValue("(iN)", kind, payload) : nullptr;
        if (!t || PyList_Append(segs, t) < 0) failed = true;
        Py_XDECREF(t);
    }
    void flush_page() {
        if (!page_items) return;
        static const char head[] = "{\"kind\":\"PodList\",\"apiVersion\":\"v1\",\"metadata\":{},\"items\":[";
        PyObject* b = PyBytes_FromStringAndSize(nullptr, (Py_ssize_t)(sizeof(head) - 1 + page.size() + 2));
        if (b) {
            char* d = PyBytes_AS_STRING(b);
            std::memcpy(d, head, sizeof(head) - 1);
            std::memcpy(d + sizeof(head) - 1, page.data(), page.size());
            std::memcpy(d + sizeof(head) - 1 + page.size(), "]}", 2);
        }
        add(0, b);
        page.clear();
        page_items = 0;
        page_uids.clear();
    }
};

// metadata.uid of a pod object (empty if absent or malformed)
std::string_view wl_uid(const Span& obj) {
    std::string_view uid;
    try {
        Parser P(obj.p, obj.p + obj.n);
        P.object([&](const char* k, size_t kn) {
            if (!uid.empty() || !KEYIS("metadata") || P.peek() != '{') {
                P.value();
                return;
            }
            P.object([&](const char* k, size_t kn) {
                Span v = P.value();
                if (KEYIS("uid") && v.is_string() && v.n >= 2) uid = std::string_view(v.p + 1, v.n - 2);
            });
        });
    } catch (const ParseError&) {
        return std::string_view();
    }
    return uid;
}

// the initial-events-end marker of a BOOKMARK object; its resourceVersion into rv
// (a repeated key counts once, the last one, at every level: as json.loads)
bool wl_end_marker(const Span& obj, std::string& rv) {
    Span md;
    Parser P(obj.p, obj.p + obj.n);
    P.object([&](const char* k, size_t kn) {
        if (KEYIS("metadata")) md = P.value(); else P.value();
    });
    if (!md.present() || md.p[0] != '{') return false;
    Span rvs, ann;
    Parser M(md.p, md.p + md.n);
    M.object([&](const char* k, size_t kn) {
        if (KEYIS("resourceVersion")) rvs = M.value();
        else if (KEYIS("annotations")) ann = M.value();
        else M.value();
    });
    if (rvs.is_string()) rv = span_text(rvs);
    return initial_events_end(ann);
}

void wl_line(WatchListObject* self, WlOut& out, const char* b, size_t n) {
    if (self->done || !n || blank(b, n)) return;
    ++self->lines;
    Span type, obj;
    try {
        bool not_object = false;
        const size_t bom = has_bom(b, n) ? 3 : 0;
        Parser P(b + bom, b + n);
        P.object([&](const char* k, size_t kn) {
            if (KEYIS("type")) {
                type = P.value();
            } else if (KEYIS("object")) {
                obj = Span();  // a repeated "object" key: the last one counts
                if (P.peek() != '{') {  // not an object: invalid, unless a later "object" key is one
                    P.value();
                    not_object = true;
                    return;
                }
                not_object = false;
                const char* st = P.p_;
                P.value();
                obj = Span{st, (size_t)(P.p_ - st)};
            } else {
                P.value();
            }
        });
        P.ws();
        if (P.p_ != P.end_) throw ParseError{"trailing data"};
        if (not_object) throw ParseError{"object is not a JSON object"};
    } catch (const ParseError& e) {
        ++self->invalid;
        out.flush_page();
        out.add(4, PyUnicode_FromFormat("%s: %.80s", e.msg, std::string(b, std::min<size_t>(n, 80)).c_str()));
        return;
    }
    const int tidx = type_index(type);
    if (tidx < 0 || !obj.present()) {
        ++self->invalid;
        out.flush_page();
        out.add(4, PyUnicode_FromString(tidx == -2 ? "unknown event type" : "missing type or object"));
        return;
    }
    if (tidx == T_ADDED || tidx == T_MODIFIED) {
        const std::string_view uid = wl_uid(obj);
        if (!uid.empty() && !out.page_uids.emplace(uid).second) {
            out.flush_page();
            out.page_uids.emplace(uid);
        }
        if (out.page_items) out.page.push_back(',');
        out.page.append(obj.p, obj.n);
        ++out.page_items;
        ++self->items;
        return;
    }
    out.flush_page();  // what came before this line applies first
    if (tidx == T_DELETED) {
        ++self->deleted;
        PyObject* line = PyBytes_FromStringAndSize(nullptr, (Py_ssize_t)n + 1);
        if (line) {
            std::memcpy(PyBytes_AS_STRING(line), b, n);
            PyBytes_AS_STRING(line)[n] = '\n';
        }
        out.add(1, line);
    } else if (tidx == T_ERROR) {
        out.add(2, PyBytes_FromStringAndSize(obj.p, (Py_ssize_t)obj.n));
        self->done = true;
    } else if (tidx == T_BOOKMARK) {
        std::string rv;
        bool end = false;
        try {
            end = wl_end_marker(obj, rv);
        } catch (const ParseError&) {
            end = false;
        }
        if (end) {
            out.add(3, PyUnicode_DecodeUTF8(rv.data(), (Py_ssize_t)rv.size(), "replace"));
            self->done = true;
        }
    }
}

// False: the stream is done (the rest of its bytes is dropped).
bool wl_segment(WatchListObject* self, WlOut& out, const char* data, size_t n) {
    if (self->done) return false;
    bool open = !self->partial->empty();
    return split_lines(data, 0, n, open, [&](uint8_t kind, size_t off, size_t len) {
        return join_line(*self->partial, kind, data + off, len, [&](const char* b, size_t blen, std::string*) {
            wl_line(self, out, b, blen);
            return !self->done;
        });
    });
}

// WatchList.feed(data, framed) -> [segments] (see above)
PyObject* WatchList_feed(WatchListObject* self, PyObject* args) {
    Py_buffer view;
    int framed;
    if (!PyArg_ParseTuple(args, "y*p", &view, &framed)) return nullptr;
    WlOut out;
    out.segs = PyList_New(0);
    if (!out.segs) {
        PyBuffer_Release(&view);
        return nullptr;
    }
    const char* data = (const char*)view.buf;
    const size_t n = (size_t)view.len;
    self->bytes += (long long)n;
    bool bad_frame = false;
    if (!framed) {
        wl_segment(self, out, data, n);
    } else if (!self->done) {  // HTTP/1.1 chunked framing (chunked.inc)
        size_t at;
        const ChunkEnd end = chunk_deframe(self->chunk, data, 0, n, at, [&](size_t off, size_t len) {
            return wl_segment(self, out, data + off, len);
        });
        bad_frame = end == CE_TOO_LONG || end == CE_BAD_SIZE;
    }
    PyBuffer_Release(&view);
    out.flush_page();
    if (bad_frame) {
        Py_DECREF(out.segs);
        PyErr_SetString(PyExc_ValueError, "WatchList: bad chunk framing");
        return nullptr;
    }
    if (out.failed) {
        Py_DECREF(out.segs);
        if (!PyErr_Occurred()) PyErr_NoMemory();
        return nullptr;
    }
    return out.segs;
}

PyObject* WatchList_stats(WatchListObject* self, PyObject*) {
    return Py_BuildValue("{s:L,s:L,s:L,s:L,s:L,s:O}", "lines", self->lines, "items", self->items, "deleted",
                         self->deleted, "invalid", self->invalid, "bytes", self->bytes, "done",
                         self->done ? Py_True : Py_False);
}

PyMethodDef WatchList_methods[] = {
    {"feed", (PyCFunction)WatchList_feed, METH_VARARGS,
     "feed(data, framed) -> [(kind, payload)]: 0 page, 1 DELETED line, 2 ERROR status, 3 end rv, 4 invalid"},
    {"stats", (PyCFunction)WatchList_stats, METH_NOARGS, "lines, items, deleted, invalid, bytes, done"},
    {nullptr, nullptr, 0, nullptr}};

PyTypeObject WatchListType = {PyVarObject_HEAD_INIT(nullptr, 0)};

int register_relist(PyObject* m) {
    WatchListType.tp_name = "_kwcore.WatchList";
    WatchListType.tp_basicsize = sizeof(WatchListObject);
    WatchListType.tp_flags = Py_TPFLAGS_DEFAULT;
    WatchListType.tp_doc = "WatchList(): a sendInitialEvents stream cut into Relist pages (see relist.inc)";
    WatchListType.tp_methods = WatchList_methods;
    WatchListType.tp_new = WatchList_new;
    WatchListType.tp_dealloc = (destructor)WatchList_dealloc;
    if (PyType_Ready(&WatchListType) < 0) return -1;
    Py_INCREF(&WatchListType);
    PyModule_AddObject(m, "WatchList", (PyObject*)&WatchListType);
    RelistType.tp_name = "_kwcore.Relist";
    RelistType.tp_basicsize = sizeof(RelistObject);
    RelistType.tp_flags = Py_TPFLAGS_DEFAULT;
    RelistType.tp_doc = "A LIST reconcile against a Pipeline's pod cache (Pipeline.relist)";
    RelistType.tp_methods = Relist_methods;
    RelistType.tp_dealloc = (destructor)Relist_dealloc;
    if (PyType_Ready(&RelistType) < 0) return -1;
    Py_INCREF(&RelistType);
    PyModule_AddObject(m, "Relist", (PyObject*)&RelistType);
    return 0;
}
