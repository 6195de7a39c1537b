"""TEST DOUBLE for the part of peclr_amd._capi that the augmenters call, in tests/_capi_double.py's style: installed only
through pytest's monkeypatch, it records every wrapper call and every attempt to reach the native library, and runs nothing.
tests/test_augment_left_host.py uses it to show that a bad `is_left` is refused BEFORE the first native call."""

WRAPPERS = ("augment_views", "augment_views_ext", "augment_views_ragged", "augment_views_ragged_ext", "supervised_labels")


class NativeCall(AssertionError):
    """A wrapper or the library itself was reached."""


def install(monkeypatch):
    """-> the list that collects the names of everything that was reached."""
    from peclr_amd import _capi

    calls = []

    def reached(name):
        def fn(*args, **kwargs):
            calls.append(name)
            raise NativeCall(name)
        return fn

    for name in WRAPPERS:
        monkeypatch.setattr(_capi, name, reached(name))
    monkeypatch.setattr(_capi, "lib", reached("lib"))
    return calls
