"""The `ref` fixture without the reference: what the reference's own compiled sources (oracle/_ref) answered to the
tests that question it, recorded call by call (tests/golden/make_golden_ref_calls.py) and checked again in the same
order where oracle/_ref cannot be built.  The tests themselves do not change: they get an object with the Ref API whose
every call must be the recorded one -- same method, same arguments (compared by a digest of dtype, shape and bytes) --
and which must be asked for every recorded answer by the end of the test.

Most answers are not stored: the oracle (tests/reflib.Oracle) has the same API, so every object handed out here is
shadowed by its oracle twin, driven with the same calls.  Where the twin's answer had the same digest (sha256 of dtype,
shape and bytes) as the reference's when the recording was made, only that digest is kept, and the answer served is
the twin's after its digest has been checked against it: bit for bit the reference's.  Answers the oracle has no
twin for, or where it differed, are stored whole.  A test that asks something else fails; it does not skip."""
import hashlib
import lzma
import os
import pickle

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
RECORDING = os.path.join(HERE, "golden", "ref_calls.pkl.xz")


class Handle:
    """an object the reference returned, by its number within the test"""

    def __init__(self, hid):
        self.hid = hid


class Same:
    """an answer equal to the oracle twin's: the digest of the reference's answer"""

    def __init__(self, digest):
        self.digest = digest


def _feed(h, v):
    if isinstance(v, np.ndarray):
        h.update(b"A" + v.dtype.str.encode() + repr(v.shape).encode() + np.ascontiguousarray(v).tobytes())
    elif isinstance(v, (tuple, list)):
        h.update(b"(" + str(len(v)).encode())
        for x in v:
            _feed(h, x)
    elif isinstance(v, dict):
        _feed(h, tuple(sorted(v.items())))
    elif isinstance(v, (bool, np.bool_)):
        h.update(b"B" + str(bool(v)).encode())
    elif isinstance(v, (int, np.integer)):
        h.update(b"I" + str(int(v)).encode())
    elif isinstance(v, (float, np.floating)):
        h.update(b"F" + np.float64(v).tobytes())
    else:
        h.update(b"V" + repr(v).encode())


def _digest(*parts):
    h = hashlib.sha256()
    _feed(h, parts)
    return h.hexdigest()[:32]


def _plain(v):
    return v is None or isinstance(v, (bool, int, float, str, bytes, np.ndarray, np.generic))


def _has_handles(v):
    if isinstance(v, (tuple, list)):
        return any(_has_handles(x) for x in v)
    return not _plain(v)


# calls of the reference whose oracle twin goes by another name
TWIN_ALIASES = {"interpolate_signal": lambda twin: (lambda iq16: twin.interp().process(iq16))}


def _twin_call(twin, name, a, kw):
    """(True, answer) of the oracle twin, or (False, None) where it has no such call or the call fails"""
    f = None
    if twin is not None:
        f = getattr(twin, name, None)
        if f is None and name in TWIN_ALIASES and hasattr(twin, "interp"):
            f = TWIN_ALIASES[name](twin)
    if f is None or not callable(f):
        return False, None
    try:
        return True, f(*a, **kw)
    except Exception:                                    # noqa: BLE001  (no twin answer: the stored one serves)
        return False, None


class _Session:
    def __init__(self):
        self.calls = {}          # test id -> [(kind, path, args digest, stored answer)]
        self.test = None
        self.n_handles = 0
        self.pos = 0             # replay: answers of the current test served so far
        self.mode = None         # "record" / "replay" / None (the live reference)

    def begin(self, test):
        self.test = test
        self.n_handles = 0
        self.pos = 0
        if self.mode == "record":
            self.calls[test] = []                        # a test run again in one session records afresh

    def finish(self):
        """replay: the test must have asked for every answer recorded for it (a loop that ends early fails)"""
        if self.mode == "replay":
            n = len(self.calls.get(self.test, []))
            assert self.pos == n, f"{self.test}: asked for {self.pos} of the {n} recorded answers of the reference"

    def peek(self):
        queue = self.calls.get(self.test) or []
        return queue[self.pos] if self.pos < len(queue) else None


class Recorder:
    """wraps the live Ref (or anything it returned) beside its oracle twin and logs every call and attribute read"""

    def __init__(self, target, twin, session, hid="ref"):
        object.__setattr__(self, "_t", target)
        object.__setattr__(self, "_twin", twin)
        object.__setattr__(self, "_s", session)
        object.__setattr__(self, "_hid", hid)

    def _encode(self, v, twin):
        """(what is stored, what the test gets) for an answer that holds handles"""
        if isinstance(v, (tuple, list)):
            pairs = [self._encode(x, t) for x, t in zip(v, twin if isinstance(twin, (tuple, list)) and len(twin) == len(v)
                                                         else [None] * len(v))]
            return tuple(p[0] for p in pairs), type(v)(p[1] for p in pairs)
        if _plain(v):
            return (v.copy() if isinstance(v, np.ndarray) else v), v
        self._s.n_handles += 1
        hid = f"h{self._s.n_handles}"
        return Handle(hid), Recorder(v, twin, self._s, hid)

    def _store(self, v, twin_ok, twin):
        """(what is stored, what the test gets): a digest where the twin's answer is the same, element by element
        inside a tuple; the answer itself elsewhere"""
        if twin_ok and not _has_handles(v) and not _has_handles(twin) and _digest(twin) == _digest(v):
            return Same(_digest(v)), v
        if twin_ok and isinstance(v, tuple) and isinstance(twin, tuple) and len(v) == len(twin):
            pairs = [self._store(x, True, t) for x, t in zip(v, twin)]
            return tuple(p[0] for p in pairs), tuple(p[1] for p in pairs)
        return self._encode(v, twin if twin_ok else None)

    def _log(self, kind, name, digest, value, twin_ok, twin_value):
        stored, live = self._store(value, twin_ok, twin_value)
        self._s.calls.setdefault(self._s.test, []).append((kind, f"{self._hid}.{name}", digest, stored))
        return live

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        v = getattr(self._t, name)
        if not callable(v):
            twin = getattr(self._twin, name, None) if self._twin is not None else None
            return self._log("attr", name, None, v, twin is not None, twin)

        def call(*a, **kw):
            ok, tv = _twin_call(self._twin, name, a, kw)
            return self._log("call", name, _digest(a, kw), v(*a, **kw), ok, tv)
        return call

    def __setattr__(self, name, value):
        setattr(self._t, name, value)

    def save(self, path=RECORDING):
        with lzma.open(path, "wb", preset=9 | lzma.PRESET_EXTREME) as f:
            pickle.dump(self._s.calls, f, protocol=4)


class Player:
    """the recorded answers, in the order the test asks for them, beside the same oracle twins as at the recording"""

    def __init__(self, session, twin, hid="ref"):
        object.__setattr__(self, "_s", session)
        object.__setattr__(self, "_twin", twin)
        object.__setattr__(self, "_hid", hid)

    def _next(self, kind, name, digest, twin_ok, twin_value):
        entry = self._s.peek()
        path = f"{self._hid}.{name}"
        assert entry is not None, f"{self._s.test}: the recording of the reference has no (further) answer for {path}"
        self._s.pos += 1
        k, p, d, stored = entry
        assert (k, p) == (kind, path), f"{self._s.test}: the test asks {kind} {path}, the recording holds {k} {p} here"
        assert digest is None or d == digest, f"{self._s.test}: {path} called with other arguments than were recorded"
        return self._decode(stored, twin_value if twin_ok else None, path)

    def _decode(self, v, twin, path):
        if isinstance(v, Same):
            assert twin is not None or v.digest == _digest(None), \
                f"{self._s.test}: {path}: the oracle gave no answer where the recording expects one"
            assert _digest(twin) == v.digest, f"{self._s.test}: {path}: the answer differs from the reference's recorded answer"
            return twin
        if isinstance(v, Handle):
            return Player(self._s, twin, v.hid)
        if isinstance(v, tuple):
            twins = twin if isinstance(twin, (tuple, list)) and len(twin) == len(v) else [None] * len(v)
            return tuple(self._decode(x, t, path) for x, t in zip(v, twins))
        return v

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        entry = self._s.peek()
        if entry is not None and entry[0] == "attr" and entry[1] == f"{self._hid}.{name}":
            twin = getattr(self._twin, name, None) if self._twin is not None else None
            return self._next("attr", name, None, twin is not None, twin)

        def call(*a, **kw):
            ok, tv = _twin_call(self._twin, name, a, kw)
            return self._next("call", name, _digest(a, kw), ok, tv)
        return call

    def __setattr__(self, name, value):
        pass                                             # (ctypes prototypes set on the library: nothing to do here)


SESSION = _Session()


def recorder(live, twin):
    SESSION.mode = "record"
    return Recorder(live, twin, SESSION)


def have_recording():
    return os.path.exists(RECORDING)


def player(twin):
    with lzma.open(RECORDING, "rb") as f:
        SESSION.calls = pickle.load(f)
    SESSION.mode = "replay"
    return Player(SESSION, twin)
