"""Replacing a file so that a reader sees the whole new one or the one before it."""

from __future__ import annotations

import os
import tempfile
from typing import Callable, TextIO


def write_atomically(path: str, write: Callable[[TextIO], None], tmp_prefix: str = ".tmp-") -> None:
    """What ``write(file)`` writes, synced under a temporary name beside
    ``path`` (its directory is made if need be), then renamed over it; the
    temporary file goes if anything fails."""
    d = os.path.dirname(os.path.abspath(path))
    os.makedirs(d, exist_ok=True)
    fd, tmp = tempfile.mkstemp(prefix=tmp_prefix, dir=d)
    try:
        with os.fdopen(fd, "w", encoding="utf-8") as f:
            write(f)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException:
        try:
            os.unlink(tmp)
        except OSError:
            pass
        raise
