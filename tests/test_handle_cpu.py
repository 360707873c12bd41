"""object_slam_amd._lib.Handle, the base of every one-handle wrapper class, over a fake library object (no GPU, no library)."""
import ctypes as C
import gc

from object_slam_amd._lib import Handle


class FakeLib:
    def __init__(self, destroy_raises=False):
        self.created, self.destroyed, self.destroy_raises = [], [], destroy_raises

    def oslam_fake_create(self, out, *args):
        out._obj.value = 0x1234
        self.created.append(args)
        return 0

    def oslam_fake_destroy(self, h):
        self.destroyed.append(h.value)
        if self.destroy_raises:
            raise RuntimeError("destroy failed")


class Fake(Handle):
    def __init__(self, L, *args):
        super().__init__(L, "oslam_fake", *args)


def test_create_passes_the_arguments_and_keeps_L_and_h():
    L = FakeLib()
    f = Fake(L, 3, 4.5)
    assert f.L is L and isinstance(f.h, C.c_void_p) and f.h.value == 0x1234 and L.created == [(3, 4.5)]
    f.close()


def test_close_twice_destroys_once():
    L = FakeLib()
    f = Fake(L)
    f.close()
    f.close()
    assert L.destroyed == [0x1234] and not f.h.value


def test_del_after_close_calls_nothing():
    L = FakeLib()
    f = Fake(L)
    f.close()
    f.__del__()
    del f
    gc.collect()
    assert L.destroyed == [0x1234]


def test_del_destroys_an_open_handle():
    L = FakeLib()
    f = Fake(L)
    del f
    gc.collect()
    assert L.destroyed == [0x1234]


def test_del_swallows_a_destroy_that_raises():
    L = FakeLib(destroy_raises=True)
    f = Fake(L)
    f.__del__()   # must not propagate
    assert L.destroyed == [0x1234]


def test_object_whose_constructor_failed_before_it_had_a_handle_can_be_collected():
    class Broken(Handle):
        def __init__(self):
            raise ValueError("before Handle.__init__")

    b = Broken.__new__(Broken)
    assert not hasattr(b, "h")
    b.close()
    b.__del__()
    try:
        Broken()
    except ValueError:
        pass
    gc.collect()
