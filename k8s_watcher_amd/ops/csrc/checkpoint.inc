// checkpoint.inc — native checkpoint (format 2): consistent snapshot on the
// event-loop thread, serialisation + fsync on another thread, native load.
// Unity-build fragment: #included into kwcore.cpp after engine.inc (it reads
// the PodCache and the NotifierCore).
//
// The reference keeps its resume point only in memory (pod_watcher.py:16), so
// a restart replays every pod as ADDED (SURVEY §5.3, §5.4). Checkpoint format
// 1 (engine/checkpoint.py) was one JSON document of the whole cache, written
// on the loop thread after pausing the watches and draining the notifier.
// Format 2 needs neither pause nor drain: PodCache.snapshot() takes, between
// two loop callbacks, (a) every cache entry's small fields into one flat
// buffer, (b) a reference to each entry's immutable payload core (CoreRef: no
// copy), and (c) a copy of every notification the notifier core still owes.
// That is a consistent cut: every event up to the scopes' resourceVersions is
// either acknowledged by clusterapi, filtered, or among the owed
// notifications, which a restart re-submits before resuming the watches. The
// snapshot is then written by CacheSnapshot.write() with the GIL released.
//
// File layout (little endian):
//   "KWCKPT02" | u32 n, header JSON (scopes, meta) | u32 n, namespace texts |
//   u32 n, phase texts | u64 n, entries | u64 n, owed notifications | u32 crc32
// text = u32 length + bytes; entry = text uid | u8 flags | text rv | text name |
//   u32 ns id | u32 phase id | text core (flags: 1 rv None, 2 name None, 4 core)
// notification = text uid | text type | text ns | text name | text body.

const char CKPT_MAGIC[8] = {'K', 'W', 'C', 'K', 'P', 'T', '0', '2'};

struct OwedNotification {
    std::string uid, etype, ns, name, body;
};

inline void ck_u32(std::string& b, uint32_t v) { b.append((const char*)&v, 4); }
inline void ck_u64(std::string& b, uint64_t v) { b.append((const char*)&v, 8); }
inline void ck_text(std::string& b, const char* p, size_t n) {
    ck_u32(b, (uint32_t)n);
    b.append(p, n);
}
inline void ck_text(std::string& b, const std::string& s) { ck_text(b, s.data(), s.size()); }

struct CacheSnapshotObject {
    PyObject_HEAD
    std::string* records;             // entries without cores, back to back
    std::vector<size_t>* ends;        // end offset of each record in `records`
    std::vector<CoreRef>* cores;      // aligned with the records (nullptr = none)
    std::vector<std::string>* ns;     // namespace id -> text
    std::vector<std::string>* phases; // phase id -> text
    std::vector<OwedNotification>* owed;
    double snap_seconds;
};

PyObject* CacheSnapshot_new(PyTypeObject* type, PyObject*, PyObject*) {
    CacheSnapshotObject* self = (CacheSnapshotObject*)type->tp_alloc(type, 0);
    if (!self) return nullptr;
    self->records = new std::string();
    self->ends = new std::vector<size_t>();
    self->cores = new std::vector<CoreRef>();
    self->ns = new std::vector<std::string>();
    self->phases = new std::vector<std::string>();
    self->owed = new std::vector<OwedNotification>();
    self->snap_seconds = 0;
    return (PyObject*)self;
}

void CacheSnapshot_dealloc(CacheSnapshotObject* self) {
    delete self->records;
    delete self->ends;
    delete self->cores;
    delete self->ns;
    delete self->phases;
    delete self->owed;
    Py_TYPE(self)->tp_free((PyObject*)self);
}

PyTypeObject CacheSnapshotType = {PyVarObject_HEAD_INIT(nullptr, 0)};

// PodCache.snapshot(notifier=None) -> CacheSnapshot (call on the loop thread)
PyObject* PodCache_snapshot(PodCacheObject* self, PyObject* args) {
    PyObject* notifier = Py_None;
    if (!PyArg_ParseTuple(args, "|O", &notifier)) return nullptr;
    if (notifier != Py_None && !PyObject_TypeCheck(notifier, &NotifierType)) {
        PyErr_SetString(PyExc_TypeError, "snapshot: notifier must be a _kwcore.Notifier or None");
        return nullptr;
    }
    const int64_t t0 = mono_ns();
    CacheSnapshotObject* snap = (CacheSnapshotObject*)CacheSnapshot_new(&CacheSnapshotType, nullptr, nullptr);
    if (!snap) return nullptr;
    const size_t n = self->store->size();
    snap->records->reserve(n * 96);
    snap->ends->reserve(n);
    snap->cores->reserve(n);
    std::string& r = *snap->records;
    self->store->for_each([&](const std::string& uid, const CacheEntry& e) {
        ck_text(r, uid);
        r.push_back((char)((e.rv_none ? 1 : 0) | (e.name_none ? 2 : 0) | (e.core ? 4 : 0)));
        ck_text(r, e.rv);
        ck_text(r, e.name);
        ck_u32(r, e.ns_id);
        ck_u32(r, e.phase_id);
        snap->ends->push_back(r.size());
        snap->cores->push_back(e.core);
    });
    *snap->ns = self->ns->text;
    *snap->phases = self->phases->text;
    if (notifier != Py_None) {
        NotifierCore& c = *((NotifierObject*)notifier)->core;
        std::lock_guard<std::recursive_mutex> g(c.mu);
        std::vector<std::pair<uint64_t, const NReq*>> live;
        live.reserve(c.reqs.size());
        for (const auto& kv : c.reqs) live.emplace_back(kv.first, &kv.second);
        std::sort(live.begin(), live.end(),
                  [](const std::pair<uint64_t, const NReq*>& a, const std::pair<uint64_t, const NReq*>& b) {
                      return a.first < b.first;
                  });
        snap->owed->reserve(live.size());
        for (const auto& p : live) {
            const NReq& q = *p.second;
            snap->owed->push_back({q.uid, q.etype, q.ns, q.name, q.body});
        }
    }
    snap->snap_seconds = (double)(mono_ns() - t0) * 1e-9;
    return (PyObject*)snap;
}

// Everything write() produces, through a bounded buffer and a running crc32.
struct CkWriter {
    int fd;
    std::string buf;
    uLong crc = crc32(0L, Z_NULL, 0);
    size_t total = 0;
    std::string err;
    explicit CkWriter(int f) : fd(f) { buf.reserve(4 << 20); }
    bool flush() {
        size_t off = 0;
        while (off < buf.size()) {
            ssize_t k = ::write(fd, buf.data() + off, buf.size() - off);
            if (k < 0 && errno == EINTR) continue;
            if (k <= 0) {
                err = std::string("write: ") + std::strerror(errno);
                return false;
            }
            off += (size_t)k;
        }
        crc = crc32(crc, (const Bytef*)buf.data(), (uInt)buf.size());
        total += buf.size();
        buf.clear();
        return true;
    }
    bool maybe_flush() { return buf.size() < (4u << 20) || flush(); }
};

// CacheSnapshot.write(path, header: bytes) -> (bytes, seconds). Releases the GIL:
// temp file in the same directory, fsync, rename over `path`, fsync the directory.
PyObject* CacheSnapshot_write(CacheSnapshotObject* self, PyObject* args) {
    const char* path;
    Py_buffer header;
    if (!PyArg_ParseTuple(args, "sy*", &path, &header)) return nullptr;
    std::string hdr((const char*)header.buf, (size_t)header.len);
    PyBuffer_Release(&header);
    // a temp name of its own per write: two writes of this process (a periodic
    // one still running when shutdown writes the final one) never share an inode
    static std::atomic<uint64_t> write_seq{0};
    std::string dst(path), tmp = dst + ".tmp-" + std::to_string((long)getpid()) + "-" + std::to_string(++write_seq);
    std::string dir = dst.find('/') == std::string::npos ? std::string(".") : dst.substr(0, dst.rfind('/'));
    if (dir.empty()) dir = "/";
    std::string err;
    size_t total = 0;
    const int64_t t0 = mono_ns();
    Py_BEGIN_ALLOW_THREADS
    int fd = ::open(tmp.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0600);
    if (fd < 0) {
        err = std::string("open ") + tmp + ": " + std::strerror(errno);
    } else {
        CkWriter w(fd);
        std::string& b = w.buf;
        b.append(CKPT_MAGIC, 8);
        ck_text(b, hdr);
        ck_u32(b, (uint32_t)self->ns->size());
        for (const auto& s : *self->ns) ck_text(b, s);
        ck_u32(b, (uint32_t)self->phases->size());
        for (const auto& s : *self->phases) ck_text(b, s);
        ck_u64(b, (uint64_t)self->ends->size());
        size_t start = 0;
        bool ok = true;
        for (size_t i = 0; i < self->ends->size() && ok; ++i) {
            const size_t end = (*self->ends)[i];
            b.append(self->records->data() + start, end - start);
            start = end;
            const CoreRef& core = (*self->cores)[i];
            if (core) ck_text(b, *core); else ck_u32(b, 0);
            ok = w.maybe_flush();
        }
        if (ok) {
            ck_u64(b, (uint64_t)self->owed->size());
            for (const auto& o : *self->owed) {
                ck_text(b, o.uid);
                ck_text(b, o.etype);
                ck_text(b, o.ns);
                ck_text(b, o.name);
                ck_text(b, o.body);
                if (!(ok = w.maybe_flush())) break;
            }
        }
        if (ok) ok = w.flush();
        if (ok) {
            uint32_t crc = (uint32_t)w.crc;
            ok = ::write(fd, &crc, 4) == 4;
            total = w.total + 4;
            if (!ok) w.err = std::string("write crc: ") + std::strerror(errno);
        }
        if (ok && ::fsync(fd) != 0) {
            ok = false;
            w.err = std::string("fsync: ") + std::strerror(errno);
        }
        ::close(fd);
        if (ok && ::rename(tmp.c_str(), dst.c_str()) != 0) {
            ok = false;
            w.err = std::string("rename: ") + std::strerror(errno);
        }
        if (ok) {
            int dfd = ::open(dir.c_str(), O_RDONLY | O_DIRECTORY | O_CLOEXEC);
            if (dfd >= 0) {
                ::fsync(dfd);  // the rename itself survives a crash
                ::close(dfd);
            }
        } else {
            ::unlink(tmp.c_str());
            err = w.err;
        }
    }
    Py_END_ALLOW_THREADS
    if (!err.empty()) {
        PyErr_SetString(PyExc_OSError, err.c_str());
        return nullptr;
    }
    return Py_BuildValue("(nd)", (Py_ssize_t)total, (double)(mono_ns() - t0) * 1e-9);
}

PyObject* CacheSnapshot_stats(CacheSnapshotObject* self, PyObject*) {
    size_t core_bytes = 0;
    for (const auto& c : *self->cores)
        if (c) core_bytes += c->size();
    size_t owed_bytes = 0;
    for (const auto& o : *self->owed) owed_bytes += o.body.size();
    return Py_BuildValue("{snsnsnsnsnsd}", "entries", (Py_ssize_t)self->ends->size(), "record_bytes",
                         (Py_ssize_t)self->records->size(), "core_bytes", (Py_ssize_t)core_bytes, "owed",
                         (Py_ssize_t)self->owed->size(), "owed_bytes", (Py_ssize_t)owed_bytes, "snapshot_seconds",
                         self->snap_seconds);
}

// CacheSnapshot.owed() -> [(uid, type, ns, name, body)]: the cut's owed
// notifications, as load_checkpoint returns them from the file write() makes
PyObject* CacheSnapshot_owed(CacheSnapshotObject* self, PyObject*) {
    PyObject* owed = PyList_New((Py_ssize_t)self->owed->size());
    if (!owed) return nullptr;
    for (size_t i = 0; i < self->owed->size(); ++i) {
        const OwedNotification& o = (*self->owed)[i];
        PyObject* item = Py_BuildValue("(s#s#s#s#y#)", o.uid.data(), (Py_ssize_t)o.uid.size(), o.etype.data(),
                                       (Py_ssize_t)o.etype.size(), o.ns.data(), (Py_ssize_t)o.ns.size(),
                                       o.name.data(), (Py_ssize_t)o.name.size(), o.body.data(),
                                       (Py_ssize_t)o.body.size());
        if (!item) {
            Py_DECREF(owed);
            return nullptr;
        }
        PyList_SET_ITEM(owed, (Py_ssize_t)i, item);
    }
    return owed;
}

PyMethodDef CacheSnapshot_methods[] = {
    {"write", (PyCFunction)CacheSnapshot_write, METH_VARARGS,
     "write(path, header_json: bytes) -> (bytes, seconds); GIL released, atomic rename"},
    {"stats", (PyCFunction)CacheSnapshot_stats, METH_NOARGS, "{entries, record_bytes, core_bytes, owed, ...}"},
    {"owed", (PyCFunction)CacheSnapshot_owed, METH_NOARGS, "[(uid, type, ns, name, body)] the notifier still owed"},
    {nullptr, nullptr, 0, nullptr}};

// ----------------------------------------------------------------------------- load

struct CkReader {
    const char* p;
    const char* e;
    bool ok = true;
    bool need(size_t n) {
        if (!ok || (size_t)(e - p) < n) ok = false;
        return ok;
    }
    uint32_t u32() {
        uint32_t v = 0;
        if (need(4)) {
            std::memcpy(&v, p, 4);
            p += 4;
        }
        return v;
    }
    uint64_t u64() {
        uint64_t v = 0;
        if (need(8)) {
            std::memcpy(&v, p, 8);
            p += 8;
        }
        return v;
    }
    uint8_t u8() {
        uint8_t v = 0;
        if (need(1)) v = (uint8_t)*p++;
        return v;
    }
    std::string text() {
        uint32_t n = u32();
        if (!need(n)) return std::string();
        std::string s(p, n);
        p += n;
        return s;
    }
};

// PodCache.load_checkpoint(path) -> (header: bytes, owed: [(uid, type, ns, name, body)])
// Adds the file's entries to this cache; ValueError on a damaged or foreign file.
PyObject* PodCache_load_checkpoint(PodCacheObject* self, PyObject* args) {
    const char* path;
    if (!PyArg_ParseTuple(args, "s", &path)) return nullptr;
    std::string data, err;
    Py_BEGIN_ALLOW_THREADS
    int fd = ::open(path, O_RDONLY | O_CLOEXEC);
    if (fd < 0) {
        err = std::string("open: ") + std::strerror(errno);
    } else {
        char buf[1 << 16];
        for (;;) {
            ssize_t k = ::read(fd, buf, sizeof buf);
            if (k < 0 && errno == EINTR) continue;
            if (k < 0) {
                err = std::string("read: ") + std::strerror(errno);
                break;
            }
            if (k == 0) break;
            data.append(buf, (size_t)k);
        }
        ::close(fd);
    }
    Py_END_ALLOW_THREADS
    if (!err.empty()) {
        PyErr_SetString(PyExc_OSError, err.c_str());
        return nullptr;
    }
    if (data.size() < 12 || std::memcmp(data.data(), CKPT_MAGIC, 8) != 0) {
        PyErr_SetString(PyExc_ValueError, "not a format-2 checkpoint");
        return nullptr;
    }
    uint32_t want;
    std::memcpy(&want, data.data() + data.size() - 4, 4);
    // in chunks: zlib's length is a 32-bit uInt, and a file past 4 GiB must not wrap it
    uLong crc = crc32(0L, Z_NULL, 0);
    for (size_t off = 0, len = data.size() - 4; off < len;) {
        const size_t k = std::min<size_t>(len - off, (size_t)1 << 30);
        crc = crc32(crc, (const Bytef*)data.data() + off, (uInt)k);
        off += k;
    }
    if ((uint32_t)crc != want) {
        PyErr_SetString(PyExc_ValueError, "checkpoint checksum mismatch (torn or damaged file)");
        return nullptr;
    }
    CkReader rd{data.data() + 8, data.data() + data.size() - 4};
    std::string header = rd.text();
    std::vector<uint32_t> ns_map, ph_map;
    for (uint32_t i = 0, n = rd.u32(); rd.ok && i < n; ++i) {
        std::string t = rd.text();
        ns_map.push_back(i == 0 ? 0 : self->ns->intern(t));
    }
    for (uint32_t i = 0, n = rd.u32(); rd.ok && i < n; ++i) {
        std::string t = rd.text();
        ph_map.push_back(i == 0 ? 0 : self->phases->intern(t));
    }
    const uint64_t n = rd.u64();
    if (rd.ok && n < (data.size() / 16)) self->store->reserve((size_t)n);  // the tables at size: no rehashes
    for (uint64_t i = 0; rd.ok && i < n; ++i) {
        std::string uid = rd.text();
        uint8_t flags = rd.u8();
        CacheEntry e;
        e.rv = rd.text();
        e.name = rd.text();
        uint32_t ns = rd.u32(), ph = rd.u32();
        std::string core = rd.text();
        if (!rd.ok || ns >= ns_map.size() || ph >= ph_map.size()) {
            rd.ok = false;
            break;
        }
        e.ns_id = ns_map[ns];
        e.phase_id = ph_map[ph];
        e.rv_none = flags & 1;
        e.name_none = flags & 2;
        if (flags & 4) e.core = std::make_shared<const std::string>(std::move(core));
        store_put(*self->store, uid, std::move(e));
    }
    PyObject* owed = PyList_New(0);
    const uint64_t m = rd.u64();
    for (uint64_t i = 0; rd.ok && owed && i < m; ++i) {
        std::string u = rd.text(), t = rd.text(), s = rd.text(), nm = rd.text(), body = rd.text();
        if (!rd.ok) break;
        PyObject* item = Py_BuildValue("(s#s#s#s#y#)", u.data(), (Py_ssize_t)u.size(), t.data(), (Py_ssize_t)t.size(),
                                       s.data(), (Py_ssize_t)s.size(), nm.data(), (Py_ssize_t)nm.size(), body.data(),
                                       (Py_ssize_t)body.size());
        if (!item || PyList_Append(owed, item) < 0) {
            Py_XDECREF(item);
            Py_CLEAR(owed);
            break;
        }
        Py_DECREF(item);
    }
    if (!owed) return nullptr;
    if (!rd.ok || rd.p != rd.e) {
        Py_DECREF(owed);
        PyErr_SetString(PyExc_ValueError, "checkpoint structure damaged");
        return nullptr;
    }
    return Py_BuildValue("(y#N)", header.data(), (Py_ssize_t)header.size(), owed);
}

int register_checkpoint(PyObject* m) {
    CacheSnapshotType.tp_name = "_kwcore.CacheSnapshot";
    CacheSnapshotType.tp_basicsize = sizeof(CacheSnapshotObject);
    CacheSnapshotType.tp_flags = Py_TPFLAGS_DEFAULT;
    CacheSnapshotType.tp_doc = "A consistent pod-cache + owed-notifications snapshot (PodCache.snapshot)";
    CacheSnapshotType.tp_methods = CacheSnapshot_methods;
    CacheSnapshotType.tp_dealloc = (destructor)CacheSnapshot_dealloc;
    if (PyType_Ready(&CacheSnapshotType) < 0) return -1;
    Py_INCREF(&CacheSnapshotType);
    PyModule_AddObject(m, "CacheSnapshot", (PyObject*)&CacheSnapshotType);
    return 0;
}
