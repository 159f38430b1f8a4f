"""HTTP/1.1 chunked de-framing and NDJSON line splitting of the four native
watch-stream consumers, on one small corpus: ``StreamDecoder.feed_chunked``,
``Pipeline.feed_chunked`` (loop-side framing), the reader hub's framing after
``take_dispatch`` handed it the pipeline's state, and ``WatchList.feed(data,
True)``; valid framings also go through the Python twin
(``PyDecoder.feed_chunked``).

Every framing is fed whole, cut in two at every byte offset and one byte per
feed; what comes out must not depend on the cut. For the hub a two-piece cut is
the hand-over itself: the pipeline frames the first piece, the hub the second,
so every offset puts another state (a size line cut mid-way, a line cut
mid-way, ``cremain`` > 0, a trailer) in the hand-over.

Pinned as they are, where the consumers differ:

* a framing error raises ``ValueError`` with the text ``chunk size line too
  long`` / ``bad chunk size line <line>`` from the decoder, the pipeline and
  the hub, and ``WatchList: bad chunk framing`` from ``WatchList``;
* the pipeline and the hub apply the lines before the error in the same feed
  (the cache has them; submits returned to Python go with the exception), the
  decoder and ``WatchList`` count them (``stats()``) and drop their results
  with the exception;
* a size line that is not UTF-8 shows with replacement characters in the
  decoder's and the pipeline's text;
* once a hub-bound body has ended, every later read of it reports the end
  again (the reflector closes the stream at the first);
* ``WatchList`` has no ``body_done``; its stream is closed when it is done.

The framings and expected lines here are also what ``scripts/chunked_check.sh``
runs through the stand-alone sanitizer build of the shared framer.
"""

import json
import os
import socket
import time

import pytest

from k8s_watcher_amd.engine.pipeline import EventPipeline
from k8s_watcher_amd.metrics import Metrics
from k8s_watcher_amd.ops.decode import PyDecoder
from k8s_watcher_amd.ops.native import NativeDecoder, load
from k8s_watcher_amd.utils.config import load_settings

ENV = "staging"  # no filter: every pod line is a submit


def _pod(etype, name, uid, rv, phase):
    return (b'{"type":"%s","object":{"metadata":{"name":"%s","namespace":"default","uid":"%s",'
            b'"resourceVersion":"%d"},"status":{"phase":"%s"}}}' % (etype, name, uid, rv, phase))


LINES = [
    _pod(b"ADDED", b"a", b"u0", 1, b"Pending"),
    _pod(b"ADDED", b"b", b"u1", 2, b"Running"),
    _pod(b"MODIFIED", b"a", b"u0", 3, b"Failed"),
    _pod(b"DELETED", b"b", b"u1", 4, b"Running"),
    b'{"type":"BOOKMARK","object":{"kind":"Pod","metadata":{"resourceVersion":"5"}}}',
    _pod(b"ADDED", b"c", b"u2", 6, b"Running"),
    _pod(b"MODIFIED", b"c", b"u2", 7, b"Succeeded"),
    _pod(b"DELETED", b"a", b"u0", 8, b"Failed"),
    _pod(b"ADDED", b"d", b"u3", 9, b"Unknown"),
]
DATA = b"".join(ln + b"\n" for ln in LINES)
END = b"0\r\n\r\n"


def _chunks(parts, head=b"%x\r\n", tail=b"\r\n"):
    return b"".join(head % len(p) + p + tail for p in parts)


def _pieces(data, n):
    return [data[i:i + n] for i in range(0, len(data), n)]


def _blank_lines():
    out = bytearray()
    for i, ln in enumerate(LINES):
        out += ln + b"\n" + (b"\n", b"  \t\r\n", b"\n\n \n", b"")[i % 4]
    return bytes(out)


_L0 = LINES[0] + b"\n"
_REST = DATA[len(_L0):]

# name -> (raw bytes, body_done once all of it is fed); every one carries LINES
FRAMINGS = {
    "chunk_per_line": (_chunks([ln + b"\n" for ln in LINES]) + END, True),
    "line_in_three_chunks": (_chunks([_L0[:40], _L0[40:41], _L0[41:], _REST]) + END, True),
    "lines_in_one_chunk": (_chunks([DATA]) + END, True),
    # chunks that end exactly at a line's end, right before its newline and right after the next one's first byte
    "chunk_ends_at_line_end": (_chunks([_L0, LINES[1], b"\n" + LINES[2] + b"\n" + LINES[3][:1],
                                        DATA[len(b"\n".join(LINES[:3])) + 2:]]) + END, True),
    "chunk_extensions": (_chunks(_pieces(DATA, 0x1a), head=b"%x;x=y\r\n") + b"0;last=\"1\"\r\n\r\n", True),
    "upper_case_hex": (_chunks(_pieces(DATA, 0xAB), head=b"%X\r\n") + END, True),
    "blanks_around_size": (_chunks(_pieces(DATA, 300), head=b" \t%x \t\r\n") + b" 0 \r\n\r\n", True),
    "bare_lf": (_chunks(_pieces(DATA, 100), head=b"%x\n", tail=b"\n") + b"0\n\n", True),
    "blank_lines_in_data": (_chunks(_pieces(_blank_lines(), 77)) + END, True),
    "trailers": (_chunks(_pieces(DATA, 500)) + b"0\r\nX-Checksum: abc\r\nX-More: 1\r\n\r\n", True),
    "bytes_after_terminator": (_chunks([DATA]) + END + b"zz\r\n" + _chunks([_L0]) + END, True),
    "no_terminator": (_chunks(_pieces(DATA, 200)), False),
}

_VALID = _chunks([b"".join(ln + b"\n" for ln in LINES[:3])])   # three lines, then the error
_AFTER = _chunks([LINES[3] + b"\n"]) + END                    # what follows it
BAD = "bad chunk size line "
LONG = "chunk size line too long"
# name -> (valid prefix, the bad size line, bytes after it, the decoder's / pipeline's / hub's text)
ERRORS = {
    "not_hex": (_VALID, b"zz\r\n", _AFTER, BAD + "zz\r"),
    "empty_size_line": (_VALID, b"\r\n", _AFTER, BAD + "\r"),
    "size_overflow": (_VALID, b"10000000000000000\r\n", _AFTER, BAD + "10000000000000000\r"),
    "size_line_too_long": (_VALID, b"1" * 5000, b"", LONG),
}
WL_ERROR = "WatchList: bad chunk framing"
N_BEFORE = 3  # lines in _VALID


def cuts_of(raw):
    """The feedings of one framing: whole, every two-piece cut, one byte per feed."""
    yield [raw]
    for k in range(1, len(raw)):
        yield [raw[:k], raw[k:]]
    yield [raw[i:i + 1] for i in range(len(raw))]


# ------------------------------------------------------------------ the consumers

def run_decoder(pieces):
    d = NativeDecoder(ENV)
    out = []
    for p in pieces:
        out += d.feed_chunked(p)
    return out, d.body_done()


def run_twin(pieces):
    d = PyDecoder(ENV)
    out = []
    for p in pieces:
        out += d.feed_chunked(p)
    return [(e[0], e[1], e[4]) for e in out], d.body_done()


_settings = None


def new_pipeline():
    from test_native_pipeline import Recorder
    global _settings
    if _settings is None:
        _settings = load_settings(ENV, environ={})
    rec = Recorder()
    p = EventPipeline(_settings, PyDecoder(ENV), rec, Metrics())
    p.log_events_setting = False
    p.attach_native()
    p.sync_native_log()
    return p, rec


def cache_of(p):
    return {u: list(e) for u, e in p.cache.items()}


def run_pipeline(pieces):
    p, rec = new_pipeline()
    ctrl = []
    for piece in pieces:
        ctrl += p.handle_raw(piece, 0, framed=True)
    return rec.calls, p.native.last_rv(), [c[0] for c in ctrl], p.native.body_done()


def flat_segments(segs):
    """WatchList segments as one sequence: a page is cut wherever a feed ends,
    its items are not."""
    out = []
    for kind, payload in segs:
        if kind == 0:
            out += [(0, item) for item in json.loads(payload)["items"]]
        else:
            out.append((kind, payload))
    return out


def run_watch_list(pieces):
    w = load().WatchList()
    segs = []
    for p in pieces:
        segs += w.feed(p, True)
    return flat_segments(segs), w.stats()


class HubRun:
    """Streams on one ReaderHub, each bound to a pipeline of its own. The first
    piece of a stream is read, taken and framed by its pipeline; take_dispatch
    then hands the framing state to the hub, which frames the rest."""

    def __init__(self, nstreams):
        self.core = load().ReaderHub(16 * 1024, max(4, 2 * nstreams))
        self.streams = {}
        self.sent = 0

    def add(self):
        a, b = socket.socketpair()
        sid = self.core.add(os.dup(b.fileno()))
        b.close()
        p, rec = new_pipeline()
        self.core.bind(sid, p.native, True)
        self.streams[sid] = {"a": a, "p": p, "rec": rec, "ctrl": [], "done": 0, "eof": False, "error": None}
        return sid

    def send(self, sid, data):
        self.streams[sid]["a"].sendall(data)
        self.sent += len(data)

    def close_write(self, sid):
        self.streams[sid]["a"].shutdown(socket.SHUT_WR)

    def wait_read(self):  # the reader thread has every byte sent so far
        deadline = time.monotonic() + 10
        while self.core.stats()["recv_bytes"] < self.sent:
            assert time.monotonic() < deadline, "the hub did not read what was sent"

    def on_item(self, it):
        sid, buf, view, read_ns, err = it
        s = self.streams[sid]
        if buf == -2:
            if isinstance(view, BaseException):
                s["error"] = s["error"] or view  # the first one
            else:
                s["ctrl"] += [e[0] for e in s["p"].native_result(view, read_ns)]
            s["done"] += bool(err)
        elif view is None:
            s["eof"] = True
        else:
            raise AssertionError(f"a bound body came back raw: {it}")

    def take(self):
        items, _ = self.core.take_dispatch()
        for it in items:
            self.on_item(it)

    def finish(self):
        """Close every stream's sending side and dispatch to each one's end;
        per stream (submits, last_rv, ctrl kinds, body_done), its error, its pipeline."""
        from test_reader_hub import _dispatch_until
        for sid in self.streams:
            self.close_write(sid)
        _dispatch_until(self.core, lambda: all(s["eof"] for s in self.streams.values()), self.on_item)
        framed = self.core.stats()["framed_reads"]
        out = {}
        for sid, s in self.streams.items():
            assert s["eof"], "stream not dispatched to its end"
            # the end of the body is reported (again by every read after it: the reflector closes the stream)
            assert bool(s["done"]) == s["p"].native.body_done()
            out[sid] = ((s["rec"].calls, s["p"].native.last_rv(), s["ctrl"], s["p"].native.body_done()),
                        s["error"], s["p"])
            self.core.unbind(sid)
            s["a"].close()
        self.core.close()
        return out, framed


def run_hub_cuts(raw, cuts, batch=48):
    """raw through the hub once per cut k: raw[:k] framed by the pipeline,
    raw[k:] by the hub. -> {k: (result, error, pipeline)}"""
    out, hub_framed = {}, 0
    for lo in range(0, len(cuts), batch):
        part = cuts[lo:lo + batch]
        hub = HubRun(len(part))
        sids = [hub.add() for _ in part]
        for sid, k in zip(sids, part):
            hub.send(sid, raw[:k])
        hub.wait_read()
        hub.take()  # ... and the hand-over
        for sid, k in zip(sids, part):
            hub.send(sid, raw[k:])
        res, framed = hub.finish()
        hub_framed += framed
        out.update({k: res[sid] for sid, k in zip(sids, part)})
    assert hub_framed > 0  # the hub did frame (not where the first piece ended the body)
    return out


def run_hub_bytewise(raw):
    """One stream, one byte per read (the hub appends them to its open buffer
    and frames each as it comes), taken every 97 bytes."""
    hub = HubRun(1)
    sid = hub.add()
    for i in range(len(raw)):
        hub.send(sid, raw[i:i + 1])
        hub.wait_read()
        if i % 97 == 0:
            hub.take()
    res, framed = hub.finish()
    assert framed > 0
    return res[sid]


# ------------------------------------------------------------------ expected, from the unframed lines

_want = {}


def want(which):
    """What each consumer makes of DATA without any framing: computed once."""
    if not _want:
        _want["decoder"] = NativeDecoder(ENV).feed(DATA)
        p, rec = new_pipeline()
        ctrl = p.handle_raw(DATA, 0, framed=False)
        _want["pipeline"] = (rec.calls, p.native.last_rv(), [c[0] for c in ctrl])
        _want["watch_list"] = flat_segments(load().WatchList().feed(DATA, False))
        _want["twin"] = [(e[0], e[1], e[4]) for e in PyDecoder(ENV).feed(DATA)]
    return _want[which]


def test_the_corpus_is_what_it_claims():
    assert len(want("decoder")) == len(LINES) == 9 and len(DATA) < 1200
    assert [e[0] for e in want("decoder")].count("BOOKMARK") == 1
    assert [(e[0], e[1], e[4]) for e in want("decoder")] == want("twin")
    calls, last_rv, ctrl = want("pipeline")
    assert len(calls) == 8 and last_rv == "9" and ctrl == []
    assert [k for k, _ in want("watch_list")] == [0, 0, 0, 1, 0, 0, 1, 0]
    for name, (raw, _done) in FRAMINGS.items():
        assert len(raw) < 1800, name


# ------------------------------------------------------------------ valid framings

@pytest.mark.parametrize("name", list(FRAMINGS))
def test_decoder_framing_at_every_cut(name):
    raw, done = FRAMINGS[name]
    for pieces in cuts_of(raw):
        assert run_decoder(pieces) == (want("decoder"), done), (name, len(pieces[0]))


@pytest.mark.parametrize("name", list(FRAMINGS))
def test_python_twin_framing_at_every_cut(name):
    raw, done = FRAMINGS[name]
    for pieces in cuts_of(raw):
        assert run_twin(pieces) == (want("twin"), done), (name, len(pieces[0]))


@pytest.mark.parametrize("name", list(FRAMINGS))
def test_pipeline_framing_at_every_cut(name):
    raw, done = FRAMINGS[name]
    for pieces in cuts_of(raw):
        assert run_pipeline(pieces) == (*want("pipeline"), done), (name, len(pieces[0]))


@pytest.mark.parametrize("name", list(FRAMINGS))
def test_watch_list_framing_at_every_cut(name):
    raw, _done = FRAMINGS[name]
    for pieces in cuts_of(raw):
        got, stats = run_watch_list(pieces)
        assert got == want("watch_list"), (name, len(pieces[0]))
        assert (stats["lines"], stats["items"], stats["deleted"], stats["invalid"]) == (9, 6, 2, 0)
        assert stats["bytes"] == len(raw) and stats["done"] is False


@pytest.mark.parametrize("name", list(FRAMINGS))
def test_hub_framing_after_a_hand_over_at_every_cut(name):
    """The pipeline frames raw[:k], take_dispatch hands its state to the hub,
    the hub frames raw[k:] — for every k, so with a size line, a data line, a
    chunk (cremain > 0), the CRLF after one and a trailer open at that moment.
    The result is the pipeline framing everything itself."""
    raw, done = FRAMINGS[name]
    for k, (got, error, _p) in run_hub_cuts(raw, list(range(1, len(raw)))).items():
        assert error is None, (name, k, error)
        assert got == (*want("pipeline"), done), (name, k)


@pytest.mark.parametrize("name", list(FRAMINGS))
def test_hub_framing_one_byte_per_read(name):
    raw, done = FRAMINGS[name]
    got, error, _p = run_hub_bytewise(raw)
    assert error is None and got == (*want("pipeline"), done)


def test_hand_over_with_each_state_open():
    """The hand-over, deterministically: a size line cut mid-way, a data line
    cut mid-way, cremain > 0 with and without a line open, and a line open
    with its chunk used up."""
    raw, done = FRAMINGS["chunk_extensions"]  # 0x1a-byte chunks under size lines "1a;x=y\r\n"
    size_line = raw.index(b"1a;x=y", 10)  # the second chunk's
    whole = FRAMINGS["lines_in_one_chunk"][0]
    exact = FRAMINGS["chunk_ends_at_line_end"][0]
    cases = [
        ("size line cut mid-way", raw, size_line + 3),
        ("size line complete but for its LF", raw, size_line + 7),
        ("line cut mid-way, cremain > 0", raw, 8 + 10),
        ("line open, between a chunk's data and its CRLF", raw, 8 + 0x1a),
        ("cremain > 0, no line open", whole, whole.index(b"\n", 10) + 1),
        ("line open, cremain == 0", exact, exact.index(LINES[1]) + len(LINES[1])),
    ]
    for what, r, k in cases:
        got, error, _p = run_hub_cuts(r, [k])[k]
        assert error is None and got == (*want("pipeline"), done), what


# ------------------------------------------------------------------ framing errors

def error_feedings(name):
    """(what, pieces, index of the piece that raises): whole, and cut before,
    inside and after the bad size line."""
    valid, bad, after, _text = ERRORS[name]
    raw = valid + bad + after
    at = len(valid)
    yield "whole", [raw], 0
    yield "cut before", [raw[:at - 30], raw[at - 30:]], 1
    yield "cut at its start", [raw[:at], raw[at:]], 1
    if name == "size_line_too_long":
        yield "cut inside", [raw[:at + 2000], raw[at + 2000:]], 1
        yield "in pieces", [raw[:at]] + _pieces(raw[at:], 1000), 5  # 4096 bytes are passed in the fifth
        yield "cut right at the limit", [raw[:at + 4096], raw[at + 4096:]], 1
    else:
        yield "cut inside", [raw[:at + 1], raw[at + 1:]], 1
        yield "cut before its LF", [raw[:at + len(bad) - 1], raw[at + len(bad) - 1:]], 1
        yield "cut after", [raw[:at + len(bad) + 5], raw[at + len(bad) + 5:]], 0
        yield "one byte per feed", [raw[i:i + 1] for i in range(at + len(bad))], at + len(bad) - 1


def lines_fed_before(pieces, upto):
    """How many of the valid prefix's lines end in pieces[:upto] (the feeds before the one that raises)."""
    return b"".join(pieces[:upto]).count(b"}\n")


@pytest.mark.parametrize("name", list(ERRORS))
def test_decoder_framing_errors(name):
    """The decoder raises the framing error's text; the events of the same
    feed go with the exception (they are counted), earlier feeds' were
    returned. After the error the size line is still there: the next feed
    raises again."""
    text = ERRORS[name][3]
    for what, pieces, bad_at in error_feedings(name):
        d = NativeDecoder(ENV)
        out = []
        for p in pieces[:bad_at]:
            out += d.feed_chunked(p)
        with pytest.raises(ValueError) as exc:
            d.feed_chunked(pieces[bad_at])
        assert str(exc.value) == text, (name, what)
        assert out == want("decoder")[:len(out)] and len(out) == lines_fed_before(pieces, bad_at), (name, what)
        assert d.stats()["events"] == N_BEFORE and not d.body_done(), (name, what)
        with pytest.raises(ValueError, match=BAD):  # the line is still there, and now ends
            d.feed_chunked(b"5\r\nhello\r\n")


@pytest.mark.parametrize("name", list(ERRORS))
def test_pipeline_framing_errors(name):
    """The pipeline applies the lines before the error — the cache has them —
    and raises; submits it would have returned from that feed go with the
    exception."""
    text = ERRORS[name][3]
    ref, _rec = new_pipeline()
    ref.handle_raw(_VALID, 0, framed=True)
    for what, pieces, bad_at in error_feedings(name):
        p, rec = new_pipeline()
        for piece in pieces[:bad_at]:
            p.handle_raw(piece, 0, framed=True)
        with pytest.raises(ValueError) as exc:
            p.handle_raw(pieces[bad_at], 0, framed=True)
        assert str(exc.value) == text, (name, what)
        assert cache_of(p) == cache_of(ref) and len(cache_of(p)) == 2, (name, what)
        assert rec.calls == want("pipeline")[0][:lines_fed_before(pieces, bad_at)], (name, what)
        assert p.native.last_rv() == "3" and not p.native.body_done(), (name, what)
        with pytest.raises(ValueError, match=BAD):  # the line is still there, and now ends
            p.handle_raw(b"5\r\nhello\r\n", 0, framed=True)


@pytest.mark.parametrize("name", list(ERRORS))
def test_watch_list_framing_errors(name):
    """WatchList raises its own text; the segments of the same feed go with
    the exception (its lines are counted)."""
    for what, pieces, bad_at in error_feedings(name):
        w = load().WatchList()
        segs = []
        for p in pieces[:bad_at]:
            segs += w.feed(p, True)
        with pytest.raises(ValueError) as exc:
            w.feed(pieces[bad_at], True)
        assert str(exc.value) == WL_ERROR, (name, what)
        got = flat_segments(segs)
        assert got == want("watch_list")[:len(got)] and len(got) == lines_fed_before(pieces, bad_at), (name, what)
        assert w.stats()["lines"] == N_BEFORE and w.stats()["done"] is False, (name, what)
        with pytest.raises(ValueError) as exc:
            w.feed(b"5\r\nhello\r\n", True)
        assert str(exc.value) == WL_ERROR


def test_a_size_line_that_is_not_utf8():
    """The decoder and the pipeline show it with replacement characters."""
    raw = _VALID + b"\xff\xfez\r\n"
    text = BAD + "\ufffd\ufffdz\r"
    with pytest.raises(ValueError) as exc:
        NativeDecoder(ENV).feed_chunked(raw)
    assert str(exc.value) == text
    p, _rec = new_pipeline()
    with pytest.raises(ValueError) as exc:
        p.handle_raw(raw, 0, framed=True)
    assert str(exc.value) == text and len(cache_of(p)) == 2
    with pytest.raises(ValueError, match=WL_ERROR):
        load().WatchList().feed(raw, True)


@pytest.mark.parametrize("name", list(ERRORS))
def test_hub_framing_errors(name):
    """Cut before or inside the bad size line, the hub finds the error and the
    read surfaces as the pipeline's ValueError, after the lines before it were
    applied; cut after it, the pipeline found it itself."""
    valid, bad, after, text = ERRORS[name]
    raw = valid + bad + after
    at = len(valid)
    ref, _rec = new_pipeline()
    ref.handle_raw(_VALID, 0, framed=True)
    cuts = [1, at - 30, at, at + 1]
    cuts += [at + 2000, at + 4096, at + 4097] if name == "size_line_too_long" else [at + len(bad) - 1, at + len(bad) + 5]
    for k, (got, error, p) in run_hub_cuts(raw, cuts).items():
        assert isinstance(error, ValueError) and str(error) == text, (name, k, error)
        assert cache_of(p) == cache_of(ref), (name, k)
        assert got[1] == "3" and got[2] == [] and got[3] is False, (name, k)
        assert got[0] == want("pipeline")[0][:len(got[0])], (name, k)
