"""clusterapi response framing: ``_kwcore.ResponseScanner`` (``scan_response``,
which also frames for the native notifier core) and its Python twin
``net/http.py::PyResponseScanner``, held to docs/DEVIATIONS.md, "Hostile
clusterapi responses" (P1-P7).

* a pinned corpus: each row states its answer (the item list, or ValueError)
  and both scanners must give it fed whole and at every split of the bytes;
* a seeded differential run against ``http.client.HTTPResponse``;
* the pools against a server that sends interim responses, chunked bodies and
  odd-sized writes: each request's fate is its own response's;
* the response that used to abort the process, sent to each pool.
"""

import asyncio
import http.client
import io
import json
import logging
import os
import random
import subprocess
import sys

import pytest

from conftest import ROOT, run
from k8s_watcher_amd.metrics import Metrics
from k8s_watcher_amd.models.payload import build_core
from k8s_watcher_amd.net.http import PyResponseScanner, parse_retry_after, response_scanner
from k8s_watcher_amd.parallel.native_notifier import NativeNotifierPool
from k8s_watcher_amd.parallel.notifier import NotifierPool
from k8s_watcher_amd.utils.config import ClusterApiSettings, NotifierPoolSettings, RetryPolicy
from k8s_watcher_amd.utils.logsetup import NOTIFIER_LOGGER

ENGINES = ("native", "python")
VE = ValueError


def scanner(engine):
    sc = response_scanner(engine == "native")
    assert (type(sc) is PyResponseScanner) == (engine == "python")
    return sc


def feed_pieces(engine, data, cuts=()):
    """Every item both feeds return, ``data`` cut at ``cuts``; ValueError as raised."""
    sc = scanner(engine)
    out = []
    prev = 0
    for c in list(cuts) + [len(data)]:
        out += sc.feed(data[prev:c])
        prev = c
    return out


# ----------------------------------------------------------------------------- pinned corpus

OK = b"HTTP/1.1 200 OK\r\nContent-Length: 2\r\n\r\nok"
H200 = b"HTTP/1.1 200 OK\r\n"
CHUNKED = H200 + b"Transfer-Encoding: chunked\r\n\r\n"


def ra(value):
    """A 503 carrying ``Retry-After: value``, then a plain 200."""
    return b"HTTP/1.1 503 Busy\r\nRetry-After:" + value + b"\r\nContent-Length: 0\r\n\r\n" + OK


def ra_items(secs):
    return [(503, True, b"", secs), 200]


PAD = b"X-Pad: " + b"a" * (65536 - len(H200) - len(b"X-Pad: ") - 4)  # head of exactly 64 KiB with its blank line


class Unframed:
    """Expected answer of a read-until-close response (P6): reported in the
    feed that completes its head, with the body bytes that feed holds."""

    def __init__(self, status, body_start, before=()):
        self.status = status
        self.body_start = body_start
        self.before = list(before)

    def items(self, data, cuts):
        end = min([c for c in cuts if c >= self.body_start] + [len(data)])
        return self.before + [(self.status, False, data[self.body_start:end], -1.0)]


# The first four rows took the process down, or wrapped around, before the
# scanner checked its arithmetic: they run in a child (test_overflow_rows_in_a_child).
CHILD_ROWS = [
    ("chunk-size-ffffffffffffffff", CHUNKED + b"ffffffffffffffff\r\nok\r\n0\r\n\r\n", VE),
    ("chunk-size-fffffffffffffffe", CHUNKED + b"fffffffffffffffe\r\nok\r\n0\r\n\r\n", VE),
    ("chunk-size-shifted-out", CHUNKED + b"10000000000000002\r\nok\r\n0\r\n\r\n", VE),
    ("content-length-wraps", H200 + b"Content-Length: 18446744073709551618\r\n\r\nok", VE),
]

ROWS = [
    # --- P2: Content-Length
    ("content-length-abc", H200 + b"Content-Length: abc\r\n\r\nok", VE),
    ("content-length-plus", H200 + b"Content-Length: +2\r\n\r\nok", VE),
    ("content-length-twice", H200 + b"Content-Length: 2\r\nContent-Length: 2\r\n\r\nok", VE),
    ("content-length-twice-differing", H200 + b"Content-Length: 2\r\ncontent-length: 3\r\n\r\nok", VE),
    ("content-length-blank-before-colon", H200 + b"Content-Length : 2\r\n\r\nok" + OK, VE),
    ("content-length-23-digits", H200 + b"Content-Length: 99999999999999999999999\r\n\r\nok", VE),
    ("content-length-2-pow-63", H200 + b"Content-Length: 9223372036854775808\r\n\r\nok", VE),
    ("content-length-2-pow-63-less-1-waits", H200 + b"Content-Length: 9223372036854775807\r\n\r\nok", []),
    ("content-length-empty", H200 + b"Content-Length: \r\n\r\n", VE),
    ("content-length-two-numbers", H200 + b"Content-Length: 2 2\r\n\r\nok", VE),
    ("content-length-list", H200 + b"Content-Length: 2, 2\r\n\r\nok", VE),
    ("content-length-underscore", H200 + b"Content-Length: 1_0\r\n\r\n0123456789", VE),
    ("content-length-hex", H200 + b"Content-Length: 0x2\r\n\r\nok", VE),
    ("content-length-superscript", H200 + b"Content-Length: \xb2\r\n\r\nok", VE),
    ("content-length-blanks-around", H200 + b"Content-Length:\t 2 \t\r\n\r\nok" + OK, [200, 200]),
    # --- P2: status line
    ("status-2000", b"HTTP/1.1 2000 OK\r\nContent-Length: 2\r\n\r\nok", VE),
    ("status-20", b"HTTP/1.1 20 OK\r\nContent-Length: 2\r\n\r\nok", VE),
    ("status-200OK", b"HTTP/1.1 200OK\r\nContent-Length: 2\r\n\r\nok", VE),
    ("status-two-blanks", b"HTTP/1.1  200 OK\r\nContent-Length: 2\r\n\r\nok", VE),
    ("status-tab", b"HTTP/1.1\t200 OK\r\nContent-Length: 2\r\n\r\nok", VE),
    ("status-signed", b"HTTP/1.1 +20 OK\r\nContent-Length: 2\r\n\r\nok", VE),
    ("status-099", b"HTTP/1.1 099 Low\r\nContent-Length: 2\r\n\r\nok", VE),
    ("status-no-reason", b"HTTP/1.1 200\r\nContent-Length: 2\r\n\r\nok", [200]),
    ("status-blank-no-reason", b"HTTP/1.1 200 \r\nContent-Length: 2\r\n\r\nok", [200]),
    ("version-2", b"HTTP/2 200\r\n\r\n", VE),
    ("version-2.0", b"HTTP/2.0 200 OK\r\nContent-Length: 2\r\n\r\nok", VE),
    ("version-1.2", b"HTTP/1.2 200 OK\r\nContent-Length: 2\r\n\r\nok", VE),
    ("version-0.9", b"HTTP/0.9 200 OK\r\nContent-Length: 2\r\n\r\nok", VE),
    ("version-lower-case", b"http/1.1 200 OK\r\nContent-Length: 2\r\n\r\nok", VE),
    ("version-missing", b"200 OK\r\nContent-Length: 2\r\n\r\nok", VE),
    ("empty-line-first", b"\r\n" + OK, VE),
    ("101-switching-protocols", b"HTTP/1.1 101 Switching Protocols\r\nUpgrade: websocket\r\n\r\n" + OK, VE),
    # --- P2: header lines
    ("blank-before-colon-any-header", H200 + b"X-Trace : 1\r\nContent-Length: 2\r\n\r\nok", VE),
    ("tab-before-colon", H200 + b"X-Trace\t: 1\r\nContent-Length: 2\r\n\r\nok", VE),
    ("folded-header-line", H200 + b"X-Trace: 1\r\n Content-Length: 2\r\nContent-Length: 2\r\n\r\nok", VE),
    ("bare-lf-in-head", H200 + b"X-Trace: 1\nContent-Length: 2\r\n\r\nok", VE),
    ("bare-cr-in-head", H200 + b"X-Trace: 1\rContent-Length: 2\r\n\r\nok", VE),
    ("line-without-colon-is-skipped", H200 + b"Content-Length\r\nContent-Length: 2\r\n\r\nok", [200]),
    # --- P2: the head's size
    ("head-64k-without-blank-line", H200 + PAD + b"aaaa", VE),
    # --- P2: chunk framing
    ("chunk-size-0x2", CHUNKED + b"0x2\r\nok\r\n0\r\n\r\n", VE),
    ("chunk-size-blanks-around", CHUNKED + b" 2 \r\nok\r\n0\r\n\r\n", VE),
    ("chunk-size-blank-in-front", CHUNKED + b" 2\r\nok\r\n0\r\n\r\n", VE),
    ("chunk-size-blanks-behind", CHUNKED + b"2 \t\r\nok\r\n0 \r\n\r\n" + OK, [200, 200]),
    ("chunk-size-blank-then-extension", CHUNKED + b"2 ;a=b\r\nok\r\n0\r\n\r\n" + OK, [200, 200]),
    ("chunk-size-g", CHUNKED + b"g\r\nok\r\n0\r\n\r\n", VE),
    ("chunk-size-minus", CHUNKED + b"-2\r\nok\r\n0\r\n\r\n", VE),
    ("chunk-size-empty", CHUNKED + b"\r\nok\r\n0\r\n\r\n", VE),
    ("chunk-size-only-extension", CHUNKED + b";a\r\nok\r\n0\r\n\r\n", VE),
    ("chunk-size-two-numbers", CHUNKED + b"2 2\r\nok\r\n0\r\n\r\n", VE),
    ("chunk-size-2-pow-63", CHUNKED + b"8000000000000000\r\nok\r\n0\r\n\r\n", VE),
    ("chunk-size-2-pow-63-less-1-waits", CHUNKED + b"7fffffffffffffff\r\nok\r\n0\r\n\r\n", []),
    ("chunk-size-leading-zeros", CHUNKED + b"000000000000000000002\r\nok\r\n0\r\n\r\n" + OK, [200, 200]),
    ("chunk-data-then-XX", CHUNKED + b"2\r\nokXX\r\n0\r\n\r\n", VE),
    ("chunk-data-then-X", CHUNKED + b"2\r\nokX\r\n0\r\n\r\n", VE),
    ("chunk-data-then-lf", CHUNKED + b"2\r\nok\n0\r\n\r\n", VE),
    ("chunk-size-line-bare-lf", CHUNKED + b"2\nok\r\n0\r\n\r\n", VE),
    ("last-chunk-bare-lf", CHUNKED + b"2\r\nok\r\n0\n\r\n", VE),
    ("trailer-end-bare-lf", CHUNKED + b"2\r\nok\r\n0\r\n\n", VE),
    ("trailer-line-bare-lf", CHUNKED + b"2\r\nok\r\n0\r\nX-T: 1\n\r\n", VE),
    ("extension-bare-lf", CHUNKED + b"2;a\nb\r\nok\r\n0\r\n\r\n", VE),
    ("chunked-error-body", b"HTTP/1.1 500 No\r\nTransfer-Encoding: chunked\r\n\r\n1;x=y\r\na\r\nA\r\nbcdefghijk\r\n00;z\r\n"
                           b"X-T: 1\r\nX-U: 2\r\n\r\n" + OK, [(500, True, b"abcdefghijk", -1.0), 200]),
    # --- P3: interim responses
    ("100-then-200", b"HTTP/1.1 100 Continue\r\n\r\n" + OK, [200]),
    ("103-with-link-then-404", b"HTTP/1.1 103 Early Hints\r\nLink: </a.css>; rel=preload\r\n\r\n"
                               b"HTTP/1.1 404 Not Found\r\nContent-Length: 2\r\n\r\nnf" + OK, [(404, True, b"nf", -1.0), 200]),
    ("102-alone", b"HTTP/1.1 102 Processing\r\n\r\n", []),
    ("100-102-103-then-200-twice", b"HTTP/1.1 100 Continue\r\n\r\nHTTP/1.1 102 Processing\r\n\r\n"
                                   b"HTTP/1.1 103 Early Hints\r\n\r\n" + OK + b"HTTP/1.1 100 Continue\r\n\r\n" + OK, [200, 200]),
    ("100-with-content-length-has-no-body", b"HTTP/1.1 100 Continue\r\nContent-Length: 2\r\n\r\n" + OK, [200]),
    ("100-closing-closes-nothing", b"HTTP/1.1 100 Continue\r\nConnection: close\r\n\r\n" + OK + OK, [200, 200]),
    # --- P4: Connection
    ("connection-close-then-keep-alive", H200 + b"Connection: close\r\nConnection: keep-alive\r\nContent-Length: 2\r\n\r\nok",
     [(200, False, b"ok", -1.0)]),
    ("connection-keep-alive-then-close", H200 + b"Connection: keep-alive\r\nconnection: Close\r\nContent-Length: 2\r\n\r\nok",
     [(200, False, b"ok", -1.0)]),
    ("connection-close-in-a-list", H200 + b"Connection: foo, CLOSE\r\nContent-Length: 2\r\n\r\nok", [(200, False, b"ok", -1.0)]),
    ("connection-1.0-keep-alive-and-close", b"HTTP/1.0 200 OK\r\nConnection: keep-alive\r\nConnection: close\r\n"
                                            b"Content-Length: 2\r\n\r\nok", [(200, False, b"ok", -1.0)]),
    ("nothing-after-a-closing-response", H200 + b"Connection: close\r\nContent-Length: 2\r\n\r\nok" + OK + b"garbage",
     [(200, False, b"ok", -1.0)]),
    # --- P5: Retry-After
    ("retry-after-1e2", ra(b" 1e2"), ra_items(-1.0)),
    ("retry-after-inf", ra(b" inf"), ra_items(-1.0)),
    ("retry-after-nan", ra(b" nan"), ra_items(-1.0)),
    ("retry-after-plus-5", ra(b" +5"), ra_items(-1.0)),
    ("retry-after-minus-5", ra(b" -5"), ra_items(-1.0)),
    ("retry-after-1_0", ra(b" 1_0"), ra_items(-1.0)),
    ("retry-after-dot-5", ra(b" .5"), ra_items(-1.0)),
    ("retry-after-hex", ra(b" 0x10"), ra_items(-1.0)),
    ("retry-after-two-numbers", ra(b" 1 2"), ra_items(-1.0)),
    ("retry-after-empty", ra(b""), ra_items(-1.0)),
    ("retry-after-twice", ra(b" 1\r\nRetry-After: 2"), ra_items(-1.0)),
    ("retry-after-twice-bad-then-good", ra(b" soon\r\nretry-after: 2"), ra_items(-1.0)),
    ("retry-after-date", ra(b" Wed, 21 Oct 2015 07:28:00 GMT"), ra_items(-1.0)),
    ("retry-after-0.25", ra(b" 0.25"), ra_items(0.25)),
    ("retry-after-0.3", ra(b"0.3"), ra_items(0.3)),
    ("retry-after-5-dot", ra(b" 5."), ra_items(5.0)),
    ("retry-after-300", ra(b" 300"), ra_items(300.0)),
    ("retry-after-301", ra(b" 301"), ra_items(300.0)),
    ("retry-after-7-in-blanks", ra(b" 7 "), ra_items(7.0)),
    ("retry-after-7-in-tabs", ra(b"\t7\t"), ra_items(7.0)),
    ("retry-after-400-digits", ra(b" " + b"9" * 400), ra_items(300.0)),
    ("retry-after-400-zeros-then-1", ra(b" 0." + b"0" * 400 + b"1"), ra_items(0.0)),
    ("retry-after-on-a-2xx-closing", H200 + b"Retry-After: 3\r\nConnection: close\r\nContent-Length: 0\r\n\r\n",
     [(200, False, b"", 3.0)]),
    # --- P6: unframed responses
    ("unframed-head-only", b"HTTP/1.1 500 Oops\r\n\r\n", [(500, False, b"", -1.0)]),
    ("unframed-with-body", b"HTTP/1.1 500 Oops\r\nX-Trace: 1\r\n\r\nit broke", Unframed(500, 33)),
    ("unframed-200-after-a-framed-one", OK + H200 + b"\r\nHTTP/1.1 200 OK\r\n\r\n", Unframed(200, len(OK) + 19, [200])),
    ("unframed-1.0", b"HTTP/1.0 200 OK\r\nConnection: keep-alive\r\n\r\nbody", Unframed(200, 43)),
    # --- P7: both framing headers
    ("chunked-and-content-length", H200 + b"Content-Length: 5\r\nTransfer-Encoding: chunked\r\n\r\n2\r\nok\r\n0\r\n\r\n" + OK,
     [200, 200]),
    ("content-length-and-chunked-error-body", b"HTTP/1.1 409 Conflict\r\nTransfer-Encoding: chunked\r\nContent-Length: 1\r\n\r\n"
                                              b"3\r\nabc\r\n0\r\n\r\n" + OK, [(409, True, b"abc", -1.0), 200]),
    ("bad-content-length-beside-chunked", H200 + b"Content-Length: x\r\nTransfer-Encoding: chunked\r\n\r\n2\r\nok\r\n0\r\n\r\n", VE),
    ("transfer-encoding-on-two-lines", H200 + b"Transfer-Encoding: gzip\r\nTransfer-Encoding: chunked\r\n\r\n2\r\nok\r\n0\r\n\r\n" + OK,
     [200, 200]),
    # --- P1: well-formed oddities
    ("204-with-content-length", b"HTTP/1.1 204 No Content\r\nContent-Length: 5\r\n\r\n" + OK, [204, 200]),
    ("304-with-content-length", b"HTTP/1.1 304 Not Modified\r\nContent-Length: 5\r\n\r\n" + OK, [(304, True, b"", -1.0), 200]),
    ("204-chunked-has-no-body", b"HTTP/1.1 204 No Content\r\nTransfer-Encoding: chunked\r\n\r\n" + OK, [204, 200]),
    ("1.0-without-connection", b"HTTP/1.0 200 OK\r\nContent-Length: 2\r\n\r\nok", [(200, False, b"ok", -1.0)]),
    ("1.0-with-keep-alive", b"HTTP/1.0 200 OK\r\nConnection: Keep-Alive\r\nContent-Length: 2\r\n\r\nok" + OK, [200, 200]),
    ("1.0-404-with-keep-alive", b"HTTP/1.0 404 No\r\nconnection: keep-alive\r\nContent-Length: 2\r\n\r\nnf" + OK,
     [(404, True, b"nf", -1.0), 200]),
    ("mixed-case-name-no-blank", H200 + b"cOnTeNt-LeNgTh:2\r\n\r\nok" + OK, [200, 200]),
    ("mixed-case-transfer-encoding", H200 + b"tRaNsFeR-eNcOdInG:CHUNKED\r\n\r\n2\r\nok\r\n0\r\n\r\n" + OK, [200, 200]),
    ("content-length-0", H200 + b"Content-Length: 0\r\n\r\n" + OK, [200, 200]),
    ("body-that-looks-like-a-response", b"HTTP/1.1 400 Bad\r\nContent-Length: 23\r\n\r\n\r\n\r\nHTTP/1.1 200 OK\r\n\r\n" + OK,
     [(400, True, b"\r\n\r\nHTTP/1.1 200 OK\r\n\r\n", -1.0), 200]),
    ("header-name-prefixes-are-other-headers", H200 + b"Content-Length-X: 9\r\nConnection-X: close\r\nX-Retry-After: 1\r\n"
                                               b"Content-Length: 2\r\n\r\nok", [200]),
]

ROW_BY_NAME = {name: (data, want) for name, data, want in CHILD_ROWS + ROWS}
assert len(ROW_BY_NAME) == len(CHILD_ROWS) + len(ROWS)


def check_row(name):
    data, want = ROW_BY_NAME[name]
    for engine in ENGINES:
        for cuts in [()] + [(k,) for k in range(1, len(data))]:
            if want is VE:
                # raised by the feed that shows the fault, or a later one; nothing reported first
                # (every such row holds one response, so P2's "never a 2xx" is "never an item")
                sc = scanner(engine)
                got = []
                with pytest.raises(ValueError):
                    prev = 0
                    for c in list(cuts) + [len(data)]:
                        got += sc.feed(data[prev:c])
                        prev = c
                    pytest.fail(f"{engine} {name} cut at {cuts}: no ValueError, items {got}")
                assert got == [], (engine, name, cuts)
            else:
                exp = want.items(data, cuts) if isinstance(want, Unframed) else want
                got = feed_pieces(engine, data, cuts)
                assert got == exp, (engine, name, cuts)
                assert [type(i) for i in got] == [type(i) for i in exp]  # 200 stays an int, bodies bytes


@pytest.mark.parametrize("name", [r[0] for r in ROWS])
def test_pinned_corpus(name):
    check_row(name)


def test_head_size_boundary():
    """Around P2's 64 KiB (the corpus row is the head that reaches it without
    its blank line): one byte less still waits, a head of exactly 64 KiB with
    its blank line is framed, one byte more is malformed. Fed whole and cut
    near both ends and at every 257th byte between: the bytes between are one
    run of padding, and the corpus row covers every cut of such a run."""
    for data, want in [(H200 + PAD + b"aaa", []),
                       (H200 + PAD + b"\r\n\r\n", [(200, False, b"", -1.0)]),
                       (H200 + PAD + b"a\r\n\r\n", VE)]:
        points = sorted(set(range(1, 64)) | set(range(64, len(data) - 64, 257)) | set(range(len(data) - 64, len(data))))
        for engine in ENGINES:
            for cuts in [()] + [(k,) for k in points]:
                if want is VE:
                    with pytest.raises(ValueError):
                        feed_pieces(engine, data, cuts)
                else:
                    assert feed_pieces(engine, data, cuts) == want, (engine, len(data), cuts)


@pytest.mark.parametrize("name", [r[0] for r in CHILD_ROWS])
def test_overflow_rows_in_a_child(name):
    """The chunk sizes that wrapped ``sz + 2`` and threw std::length_error through
    C code, and the two silent overflows. Run in a child so a regression fails
    the test, not the test run."""
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import test_response_scanner as t\n"
            "t.check_row(%r)\n"
            "print('ok')\n") % (ROOT, os.path.join(ROOT, "tests"), name)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.returncode, out.stderr[-2000:])


def test_policy_names_its_rows():
    """docs/DEVIATIONS.md, "Hostile clusterapi responses": every item P1-P7 ends
    in a "Rows:" line naming the corpus rows that pin it; every name is a row
    and every row is named."""
    import re
    text = open(os.path.join(ROOT, "docs", "DEVIATIONS.md"), encoding="utf-8").read()
    section = text.split("## Hostile clusterapi responses", 1)[1].split("\n## ", 1)[0]
    named = {}
    item = None
    for line in section.splitlines():
        m = re.match(r"- \*\*(P[1-7]) ", line)
        if m:
            item = m.group(1)
        elif line.strip().startswith("Rows:"):
            named.setdefault(item, []).extend(re.findall(r"`([^`]+)`", line))
    assert sorted(named) == ["P1", "P2", "P3", "P4", "P5", "P6", "P7"] and all(named.values())
    every = [n for names in named.values() for n in names]
    assert sorted(every) == sorted(ROW_BY_NAME), set(every) ^ set(ROW_BY_NAME)


def test_python_retry_after_follows_p5():
    """``net.http.parse_retry_after`` alone (the reflector and the compat client call it)."""
    for text, want in [("0.25", 0.25), ("300", 300.0), ("301", 300.0), (" 7 ", 7.0), ("5.", 5.0), ("0", 0.0)]:
        assert parse_retry_after(text) == want
    for text in (None, "", " ", "1e2", "inf", "nan", "+5", "-5", "1_0", ".5", "1, 2", "Wed, 21 Oct 2015 07:28:00 GMT",
                 "١", "1\n"):
        assert parse_retry_after(text) is None, text


# ----------------------------------------------------------------------------- differential run against http.client

STATUSES = (200, 201, 202, 204, 304, 400, 404, 409, 429, 500, 502, 503)
BODY_SIZES = (0, 1, 2, 15, 16, 17, 100, 700)
LOOKALIKE = b"\r\n\r\nHTTP/1.1 200 OK\r\n"
CONNECTION = (None,) * 10 + ("close", "keep-alive", "Keep-Alive", "CLOSE", "foo, close")
RETRY_AFTER = (("0", 0.0), ("1", 1.0), ("0.25", 0.25), ("2.5", 2.5), ("0.3", 0.3), ("120", 120.0), ("300", 300.0),
               ("301", 300.0), ("Wed, 21 Oct 2015 07:28:00 GMT", -1.0))
INTERIM = (b"HTTP/1.1 100 Continue\r\n\r\n", b"HTTP/1.1 102 Processing\r\n\r\n",
           b"HTTP/1.1 103 Early Hints\r\nLink: </style.css>; rel=preload\r\n\r\n")


class _FakeSocket:
    def __init__(self, data):
        self.file = io.BytesIO(data)

    def makefile(self, *_a, **_k):
        return self.file


def oracle(message, retry_after):
    """The item for ``message`` alone, framed by the standard library."""
    r = http.client.HTTPResponse(_FakeSocket(message))
    r.begin()
    body = r.read()
    keep = not r.will_close
    if 200 <= r.status < 300 and keep:
        return r.status
    return (r.status, keep, body, retry_after)


def _case(name, rng):
    return "".join(c.upper() if rng.random() < 0.5 else c.lower() for c in name)


def _header(rng, name, value):
    return f"{_case(name, rng)}:{rng.choice(('', ' ', chr(9), '  '))}{value}\r\n".encode("latin-1")


def gen_message(rng, last):
    """One well-formed message: ``(bytes, retry_after, body_start or None)``,
    ``body_start`` set for an unframed one."""
    status = rng.choice(STATUSES)
    http10 = rng.random() < 0.1
    n = rng.choice(BODY_SIZES)
    body = rng.randbytes(n)
    if n >= 100 and rng.random() < 0.3:
        at = rng.randrange(n - len(LOOKALIKE))
        body = body[:at] + LOOKALIKE + body[at + len(LOOKALIKE):]
    no_body = status in (204, 304)
    head = [f"HTTP/1.{0 if http10 else 1} {status} {rng.choice(('OK', 'Some Reason', ''))}".rstrip().encode() + b"\r\n"]
    headers = []
    conn = rng.choice(CONNECTION)
    if conn is not None:
        headers.append(_header(rng, "Connection", conn))
    retry_after = -1.0
    if status in (429, 503) and rng.random() < 0.7:
        text, retry_after = rng.choice(RETRY_AFTER)
        headers.append(_header(rng, "Retry-After", text + rng.choice(("", " ", "\t"))))
    if rng.random() < 0.5:
        headers.append(_header(rng, "Content-Type", "application/json"))
    payload = b""
    unframed = False
    if no_body:
        if rng.random() < 0.5:
            headers.append(_header(rng, "Content-Length", str(rng.choice((0, 5)))))
    elif last and n and rng.random() < 0.3:
        unframed = True
        payload = body
    elif not http10 and rng.random() < 0.5:
        headers.append(_header(rng, "Transfer-Encoding", rng.choice(("chunked", "Chunked", "CHUNKED"))).rstrip() + b"\r\n")
        if rng.random() < 0.2:  # P7: chunked wins
            headers.append(_header(rng, "Content-Length", str(rng.choice((0, n, n + 3)))))
        parts = []
        off = 0
        while off < n:
            k = min(rng.choice((1, 3, 16, 255, 4096)), n - off)
            size = rng.choice(("%x", "%X", "0%x"))  % k
            ext = rng.choice(("", "", ";a=b", ";z", " ;q"))
            parts.append(size.encode() + ext.encode() + b"\r\n" + body[off:off + k] + b"\r\n")
            off += k
        parts.append(rng.choice((b"0", b"00", b"0;z")) + b"\r\n")
        for _ in range(rng.randrange(3)):
            parts.append(_header(rng, "X-Trailer", "t"))
        parts.append(b"\r\n")
        payload = b"".join(parts)
    else:
        headers.append(_header(rng, "Content-Length", str(n) + rng.choice(("", " "))))
        payload = body
    rng.shuffle(headers)
    head_bytes = b"".join(head + headers) + b"\r\n"
    return head_bytes + payload, retry_after, (len(head_bytes) if unframed else None)


def closes(item):
    return not isinstance(item, int) and not item[1]


def gen_case(rng):
    """1-6 pipelined messages, ending at the first that closes:
    ``[(bytes, expected item, body_start or None)]``."""
    out = []
    count = rng.randint(1, 6)
    for i in range(count):
        msg, retry_after, body_start = gen_message(rng, last=i == count - 1)
        item = oracle(msg, retry_after)
        out.append((msg, item, body_start))
        if closes(item):
            break
    return out


def assemble(rng, case, interim):
    """The case's bytes and its expected items as a function of the cuts."""
    data = b""
    items = []
    unframed_at = None
    for msg, item, body_start in case:
        while interim and rng.random() < 0.4:
            data += rng.choice(INTERIM)
        if body_start is not None:
            unframed_at = len(data) + body_start
        data += msg
        items.append(item)
    return data, items, unframed_at


def expected_for(data, items, unframed_at, cuts):
    if unframed_at is None:
        return items
    status, keep, _body, retry_after = items[-1]
    assert not keep
    end = min([c for c in cuts if c >= unframed_at] + [len(data)])
    return items[:-1] + [(status, False, data[unframed_at:end], retry_after)]  # P6


FUZZ_CASES = 3000


def test_differential_against_http_client():
    """Seeded, unfiltered: every generated case is compared. ``http.client``
    frames each message alone; both scanners must give the same items for the
    pipelined bytes, with and without interim responses in front of the
    messages (P3), cut at 0 / 1 / 2 / 5 random points. An unframed last
    message is expected as P6 reports it: in the feed that completes its
    head."""
    rng = random.Random(20251020)
    seen = {"unframed": 0, "chunked": 0, "closing": 0, "interim": 0, "non_2xx": 0, "messages": 0}
    for n in range(FUZZ_CASES):
        case = gen_case(rng)
        seen["messages"] += len(case)
        seen["chunked"] += sum(b"chunked" in m.lower().split(b"\r\n\r\n")[0] for m, _i, _b in case)
        seen["closing"] += closes(case[-1][1])
        seen["non_2xx"] += sum(not isinstance(i, int) for _m, i, _b in case)
        for interim in (False, True):
            data, items, unframed_at = assemble(rng, case, interim)
            seen["interim"] += interim and data.count(b"HTTP/1.1 10") > 0
            seen["unframed"] += unframed_at is not None
            cuts = sorted(rng.sample(range(1, len(data)), min(rng.choice((0, 1, 2, 5)), len(data) - 1)))
            want = expected_for(data, items, unframed_at, cuts)
            for engine in ENGINES:
                got = feed_pieces(engine, data, cuts)
                assert got == want, (n, engine, interim, cuts, data)
    # the generator reached what it is there for
    assert seen["messages"] > 2 * FUZZ_CASES and min(seen.values()) > FUZZ_CASES // 10, seen


# ----------------------------------------------------------------------------- pool level

TS = "2025-01-01T00:00:00.000001"
POOLS = ("python", "python-native-scanner", "native", "native-io-thread")


def make_pool(kind, url, metrics, connections=2, depth=4):
    pool = NotifierPoolSettings(connections=connections, pipeline_depth=depth, queue_size=1000, coalesce=False,
                                io_thread="on" if kind == "native-io-thread" else "off")
    s = ClusterApiSettings(base_url=url, pool=pool, retry=RetryPolicy(4, 0.002, 2.0, 0.02, 0.0), timeout=10.0)
    if kind.startswith("python"):
        return NotifierPool(s, metrics, native=kind == "python-native-scanner")
    return NativeNotifierPool(s, metrics)


def core(uid):
    pod = {"metadata": {"name": f"pod-{uid}", "namespace": "default", "uid": uid}, "status": {"phase": "Running"}}
    return build_core(pod, "production")


class ScriptedServer:
    """A raw clusterapi stand-in: reads pipelined POSTs and answers them one by
    one with ``script(uid, attempt)``'s bytes, written in odd-sized pieces."""

    PIECES = (1, 7, 3, 13, 2, 29, 5)

    def __init__(self, script):
        self.script = script
        self.requests = []      # (connection number, uid), in arrival order
        self.attempts = {}
        self.connections = 0
        self.server = None

    async def start(self):
        self.server = await asyncio.start_server(self.serve, "127.0.0.1", 0)
        self.url = "http://127.0.0.1:%d" % self.server.sockets[0].getsockname()[1]

    async def stop(self):
        self.server.close()
        await self.server.wait_closed()

    async def serve(self, reader, writer):
        self.connections += 1
        number = self.connections
        try:
            while True:
                head = await reader.readuntil(b"\r\n\r\n")
                assert head.startswith(b"POST "), head
                length = int([ln.split(b":")[1] for ln in head.split(b"\r\n") if ln.lower().startswith(b"content-length:")][0])
                uid = json.loads(await reader.readexactly(length))["uid"]
                attempt = self.attempts[uid] = self.attempts.get(uid, 0) + 1
                self.requests.append((number, uid))
                answer = self.script(uid, attempt)
                off = 0
                k = len(self.requests)
                while off < len(answer):
                    size = self.PIECES[k % len(self.PIECES)]
                    k += 1
                    writer.write(answer[off:off + size])
                    off += size
                    await writer.drain()
                    if k % 3 == 0:
                        await asyncio.sleep(0)  # let the pool read a partial response
        except (asyncio.IncompleteReadError, ConnectionError):
            pass
        finally:
            writer.close()


class _Records(logging.Handler):
    def __init__(self):
        super().__init__(logging.ERROR)
        self.messages = []

    def emit(self, record):
        self.messages.append(record.getMessage())


N_UIDS = 64


def kind_of(i):
    return "busy-once" if i % 4 == 1 else "gone" if i % 8 == 3 else "fine"


def fates_script(uid, attempt):
    i = int(uid[1:])
    kind = kind_of(i)
    if kind == "busy-once" and attempt == 1:
        answer = b"HTTP/1.1 503 Service Unavailable\r\nRetry-After: 0\r\nContent-Length: 4\r\n\r\nbusy"
    elif kind == "gone":
        answer = b"HTTP/1.1 404 Not Found\r\nContent-Length: 7\r\n\r\nno such"
    elif i % 3 == 0:
        answer = b"HTTP/1.1 200 OK\r\nTransfer-Encoding: chunked\r\n\r\n1;x\r\n{\r\n1\r\n}\r\n0\r\nX-T: 1\r\n\r\n"
    else:
        answer = b"HTTP/1.1 200 OK\r\nContent-Length: 2\r\n\r\n{}"
    if (i + attempt) % 2 == 0:  # half of all answers: an interim response first
        interim = (b"HTTP/1.1 100 Continue\r\n\r\n" if i % 4 < 2 else
                   b"HTTP/1.1 103 Early Hints\r\nLink: </x>; rel=preload\r\n\r\n")
        answer = interim + answer
    return answer


def check_each_request_gets_its_own_answer(kind):
    """64 uids over 2 connections, 4 deep: a quarter answered 503 then 200, an
    eighth 404, the rest 200 (some chunked), half of all answers behind a 100
    or a 103. Delivered, failed, retried and logged must be exactly what the
    script gave each uid."""
    uids = [f"u{i}" for i in range(N_UIDS)]
    busy = [u for i, u in enumerate(uids) if kind_of(i) == "busy-once"]
    gone = [u for i, u in enumerate(uids) if kind_of(i) == "gone"]
    assert len(busy) == 16 and len(gone) == 8

    async def body():
        srv = ScriptedServer(fates_script)
        await srv.start()
        m = Metrics()
        pool = make_pool(kind, srv.url, m)
        for u in uids:
            pool.submit(u, "ADDED", "default", f"pod-{u}", core(u), 0, TS)
        pool.flush()
        drained = await pool.drain(20)
        await pool.close()
        await srv.stop()
        return drained, m, srv

    records = _Records()
    log = logging.getLogger(NOTIFIER_LOGGER)
    log.addHandler(records)
    try:
        drained, m, srv = run(body())
    finally:
        log.removeHandler(records)
    assert drained, (m.c["notify_delivered"], m.c["notify_failed"])  # no request left without an answer
    assert m.c["notify_delivered"] == N_UIDS - len(gone)
    assert m.c["notify_failed"] == len(gone)
    seen = {}
    for _conn, uid in srv.requests:
        seen[uid] = seen.get(uid, 0) + 1
    assert seen == {u: 2 if u in busy else 1 for u in uids}
    assert srv.connections == 2
    statuses = [msg.split("Status: ")[1].split(",")[0] for msg in records.messages if "Status: " in msg]
    assert sorted(statuses) == ["404"] * len(gone) + ["503"] * len(busy), records.messages
    assert not [msg for msg in records.messages if "Status: " not in msg], records.messages


@pytest.mark.parametrize("kind", POOLS)
def test_each_request_gets_its_own_answer(kind):
    check_each_request_gets_its_own_answer(kind)


ABORT_ANSWER = b"HTTP/1.1 200 OK\r\nTransfer-Encoding: chunked\r\n\r\nffffffffffffffff\r\nok\r\n0\r\n\r\n"


def check_overflowing_chunk_at_pool(kind):
    """Child-process body of test_overflowing_chunk_drops_the_connection."""
    def script(_uid, attempt):
        return ABORT_ANSWER if attempt == 1 else b"HTTP/1.1 200 OK\r\nContent-Length: 2\r\n\r\n{}"

    async def body():
        srv = ScriptedServer(script)
        await srv.start()
        m = Metrics()
        pool = make_pool(kind, srv.url, m, connections=1, depth=1)
        pool.submit("u0", "ADDED", "default", "pod-u0", core("u0"), 0, TS)
        pool.flush()
        drained = await pool.drain(20)
        await pool.close()
        await srv.stop()
        return drained, m, srv

    records = _Records()
    log = logging.getLogger(NOTIFIER_LOGGER)
    log.addHandler(records)
    drained, m, srv = run(body())
    log.removeHandler(records)
    assert drained
    assert m.c["notify_delivered"] == 1 and m.c["notify_failed"] == 0 and m.c["notify_retried"] == 1
    assert srv.requests == [(1, "u0"), (2, "u0")]  # retried on a new connection
    assert any(msg.startswith("Unexpected error calling clusterapi") for msg in records.messages), records.messages


@pytest.mark.parametrize("kind", POOLS)
def test_overflowing_chunk_drops_the_connection(kind):
    """The response that ended the process (chunk size ffffffffffffffff): the
    connection is dropped, the error logged, the request retried on a new
    connection and delivered. In a child so a regression fails, not aborts."""
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import test_response_scanner as t\n"
            "t.check_overflowing_chunk_at_pool(%r)\n"
            "print('ok')\n") % (ROOT, os.path.join(ROOT, "tests"), kind)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.returncode, out.stderr[-2000:])
