"""The files of the hand-over directory (parallel/shard.py), byte for byte:
shards of two versions share the directory during a rolling update, so the
record codec may be rearranged but what it writes may not change. The rows
that tests/test_sharding.py (test_handover_record_roundtrip) and
tests/test_parting.py already assert are not repeated here."""

import json
import os
import types

import pytest
from k8s_watcher_amd.parallel import shard
from k8s_watcher_amd.parallel.shard import (discard_parting, read_manifest, record_layout, take_handover, take_parting,
                                            write_handover, write_manifest, write_parting)

NOW = 1700000000.25
PODS = [("uid-1", "7", "Running", "pod-é", '{"name":"pod-é","phase":"Running"}'.encode("utf-8")),
        ("uid-2", None, None, "pod-2", None)]
OWED = [("uid-1", "MODIFIED", "ns-a", "pod-é", b'{"n":1}\xff\x00')]
LAYOUT = {"count": 3, "assignment": "hash", "key": "namespace"}
BEFORE = {"count": 2, "assignment": "hash", "key": "namespace"}

# What the functions wrote for the input above before there was one codec
# (generated with them, from the commit before that change, time.time pinned to NOW)
HANDOVER = (b'{"version":2,"namespace":"ns-a","from":2,"to":0,"written_at":1700000000.25,"layout":{"count":3,'
            b'"assignment":"hash","key":"namespace"},"pods":[["uid-1","7","Running","pod-\\u00e9",'
            b'"{\\"name\\":\\"pod-\\u00e9\\",\\"phase\\":\\"Running\\"}"],["uid-2",null,null,"pod-2",null]],'
            b'"owed":[["uid-1","MODIFIED","ns-a","pod-\\u00e9","eyJuIjoxff8A"]]}')
PARTING = HANDOVER.replace(b'"from":2,"to":0,', b'"from":2,')
MANIFEST = (b'{"version": 2, "shard": 2, "layout": {"count": 3, "assignment": "hash", "key": "namespace"}, '
            b'"written_at": 1700000000.25, "namespaces": ["ns-a", "ns-b"]}')
LAYOUT_JSON = (b'{"current": {"count": 3, "assignment": "hash", "key": "namespace"}, "previous": {"count": 2, '
               b'"assignment": "hash", "key": "namespace"}, "since": 1700000000.25}')


@pytest.fixture
def hdir(tmp_path, monkeypatch):
    monkeypatch.setattr(shard, "time", types.SimpleNamespace(time=lambda: NOW))  # the module's own name only
    return str(tmp_path / "handover")  # made by whoever writes first


def _bytes(path):
    with open(path, "rb") as f:
        return f.read()


def test_the_four_files_are_what_they_were_byte_for_byte(hdir):
    assert _bytes(write_handover(hdir, "ns-a", 2, 0, PODS, OWED, LAYOUT)) == HANDOVER
    assert _bytes(write_parting(hdir, "ns-a", 2, PODS, OWED, LAYOUT)) == PARTING
    assert _bytes(write_manifest(hdir, 2, LAYOUT, ["ns-b", "ns-a"])) == MANIFEST
    assert record_layout(hdir, BEFORE) == (None, NOW)
    assert record_layout(hdir, LAYOUT) == (BEFORE, NOW)
    assert _bytes(os.path.join(hdir, "layout.json")) == LAYOUT_JSON
    # no temporary file left beside them
    assert sorted(os.listdir(hdir)) == ["layout.json", "ns-a.handover.json", "ns-a.parting.json", "shard-2.parted.json"]
    # a parting record stamped by its caller (part() gives every record and the manifest one time)
    assert _bytes(write_parting(hdir, "ns-a", 2, PODS, OWED, LAYOUT, written_at=5.5)) == \
        PARTING.replace(b"1700000000.25", b"5.5")
    assert _bytes(write_manifest(hdir, 2, LAYOUT, [], written_at=5.5)).endswith(b'"written_at": 5.5, "namespaces": []}')


def test_each_file_reads_back_as_what_was_written(hdir):
    # (a core that is not UTF-8 does not survive: the record carries text)
    write_handover(hdir, "ns-a", 2, 0, PODS, OWED, LAYOUT)
    rec = take_handover(hdir, "ns-a", 0, not_before=NOW, layout=LAYOUT)  # at the bound: taken
    assert (rec.pods, rec.owed, rec.src, rec.written_at) == (PODS, OWED, 2, NOW)
    write_parting(hdir, "ns-a", 2, PODS, OWED, LAYOUT)
    rec = take_parting(hdir, "ns-a", 2, not_before=NOW, layout=LAYOUT)
    assert (rec.pods, rec.owed, rec.src, rec.written_at) == (PODS, OWED, 2, NOW)
    write_parting(hdir, "ns-b", 1, [], None, None)
    assert take_parting(hdir, "ns-b", 1) == ([], [], 1, NOW)
    write_manifest(hdir, 2, LAYOUT, ["ns-b", "ns-a"])
    assert read_manifest(hdir, 2) == json.loads(MANIFEST)
    assert os.listdir(hdir) == ["shard-2.parted.json"]  # records are consumed, the manifest is read


@pytest.mark.parametrize("kind, take, left", [
    # (what is asked of the record written below: from shard 2, for shard 0, at NOW, under LAYOUT)
    ("handover", lambda d: take_handover(d, "ns-a", 0, not_before=NOW + 0.5), False),  # too old: removed
    ("parting", lambda d: take_parting(d, "ns-a", 2, not_before=NOW + 0.5, layout=LAYOUT), False),
    ("parting", lambda d: take_parting(d, "ns-a", 2, layout=BEFORE), False),  # another layout: removed
    ("parting", lambda d: take_parting(d, "ns-a", 1, layout=LAYOUT), True),  # another shard's: left
    ("parting", lambda d: discard_parting(d, "ns-a", 1) or None, True),
    ("handover", lambda d: take_handover(d, "ns-b", 0), True),  # no such record
])
def test_what_is_not_taken_is_removed_only_if_it_was_stale(hdir, kind, take, left):
    write = {"handover": lambda: write_handover(hdir, "ns-a", 2, 0, PODS, OWED, LAYOUT),
             "parting": lambda: write_parting(hdir, "ns-a", 2, PODS, OWED, LAYOUT)}[kind]
    path = write()
    assert take(hdir) is None
    assert os.path.exists(path) is left


def test_a_file_of_another_version_or_of_another_writer_is_nobodys(hdir):
    paths = [write_handover(hdir, "ns-a", 2, 0, PODS, OWED, LAYOUT), write_parting(hdir, "ns-a", 2, PODS, OWED, LAYOUT),
             write_manifest(hdir, 2, LAYOUT, ["ns-a"])]
    os.replace(paths[2], os.path.join(hdir, "shard-1.parted.json"))  # says shard 2, named as shard 1's
    assert read_manifest(hdir, 1) is None and read_manifest(hdir, 2) is None
    for path in paths[:2]:
        with open(path) as f:
            doc = json.load(f)
        doc["version"] = 1
        with open(path, "w") as f:
            json.dump(doc, f)
    assert take_handover(hdir, "ns-a", 0) is None and take_parting(hdir, "ns-a", 2) is None
    assert discard_parting(hdir, "ns-a", 2) is False
    assert sorted(os.listdir(hdir)) == ["ns-a.handover.json", "ns-a.parting.json", "shard-1.parted.json"]
    write_parting(hdir, "ns-a", 2, [], None, LAYOUT)
    assert discard_parting(hdir, "ns-a", 2) is True and not os.path.exists(paths[1])
