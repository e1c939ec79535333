"""The cases of the harness self-test (tests/guard.py), shared by tests/test_guard.py (host) and tests/test_gpu_workspace.py (device).
Every "dirty" case is a plain in-bounds torch write through the BASE tensor of a guarded allocation: nothing here overruns anything."""
import torch

from tests import guard as G

CASES = ("clean_block_passes", "front_band_byte", "back_band_byte", "layout_padding_byte", "factories_and_alignment", "poison_modes",
         "pass_through", "patches_are_put_back", "unchanged_helper", "find_and_records")


def _raises(fn, *needles):
    try:
        fn()
    except AssertionError as e:
        for n in needles:
            assert n in str(e), (n, str(e))
        return str(e)
    raise RuntimeError("the guard did not notice: " + ", ".join(needles))


def check_clean_block_passes(device):
    with G.guarded_allocations(device, poison="float_nan") as g:
        a = torch.empty(1000, 3, device=device)
        a.fill_(1.0)                                    # the whole interior, first and last byte included
        b = torch.zeros(7, dtype=torch.int32, device=device)
        b += 5
        c = a.new_empty(0)
        g.verify()
        assert len(g.allocations) == 3 and c.numel() == 0


def _one_byte(device, where):
    def run():
        with G.guarded_allocations(device) as g:
            t = torch.empty(1001, dtype=torch.float32, device=device)          # 4004 bytes: not a multiple of the alignment
            al = g.allocations[-1]
            at = al.offset - 1 if where == "front" else al.offset + al.nbytes + 5
            al.base[at] = 0                             # in bounds of the base: a band byte
            assert t.numel() == 1001
    return run


def check_front_band_byte(device):
    msg = _raises(_one_byte(device, "front"), "front band", "4004 bytes", "first at -4005, last at -4005", "guard_selftest.py")
    assert "back band" not in msg


def check_back_band_byte(device):
    msg = _raises(_one_byte(device, "back"), "back band", "4004 bytes", "first at +5, last at +5", "guard_selftest.py")
    assert "front band" not in msg


def check_layout_padding_byte(device):
    """A two-region layout the way align_up lays it out: [0, 100) used, padding to 256, [256, 256 + 300) used, padding to 768."""
    regions = [(0, 100), (256, 300)]
    with G.guarded_allocations(device) as g:
        ws = torch.full((768,), 0x5A, dtype=torch.uint8, device=device)
        ws[0:100] = 1
        ws[256:556] = 2                                 # every used byte written: passes
        assert G.check_regions(ws, 0x5A, regions) == 768 - 400
        assert G.check_regions(g.find(768)[0], 0x5A, regions) == 768 - 400
        ws[100] = 0                                     # the first padding byte behind region 0
        _raises(lambda: G.check_regions(ws, 0x5A, regions, name="two_regions"), "two_regions", "first at offset 100, last at 100", "starts at 0")
        ws[100] = 0x5A
        ws[767] = 0                                     # the last byte of the tail padding
        _raises(lambda: G.check_regions(ws, 0x5A, regions), "first at offset 767", "starts at 256")
        # a layout whose second region starts inside what the first one is described to hold
        _raises(lambda: G.check_regions(ws, 0x5A, [(0, 260), (256, 300)], name="short_layout"), "short_layout", "4 byte(s) into the region at offset 256")


def check_factories_and_alignment(device):
    with G.guarded_allocations(device) as g:
        src = torch.arange(12, dtype=torch.float32).reshape(3, 4).to(device)         # (a copy onto a GPU is itself guarded)
        first = len(g.allocations)
        made = [torch.empty(5, device=device), torch.empty((2, 3), dtype=torch.int64, device=device), torch.empty_like(src),
                torch.zeros(3, 3, device=device), torch.zeros_like(src), torch.ones(4, dtype=torch.int32, device=device),
                torch.full((3,), 7.5, device=device), torch.full_like(src, 2.0), src.new_empty(9), src.new_zeros((2, 2)), src.new_full((5,), 3.0),
                torch.empty(3, dtype=torch.bool, device=device), torch.empty((), device=device), torch.empty(1, dtype=torch.uint8, device=device),
                torch.empty_like(src.t())]
        assert len(g.allocations) == first + len(made)
        for t, al in zip(made, g.allocations[first:]):
            assert t.data_ptr() % 256 == 0 and t.is_contiguous() and t.data_ptr() == al.tensor.data_ptr(), al
            assert al.nbytes == t.numel() * t.element_size() and al.shape == tuple(t.shape) and al.dtype == t.dtype
            assert not t.requires_grad
        assert float(made[3].abs().sum()) == 0 and float(made[4].abs().sum()) == 0 and int(made[5].sum()) == 4
        assert made[6].tolist() == [7.5] * 3 and float(made[7].sum()) == 24.0 and float(made[9].abs().sum()) == 0 and made[10].tolist() == [3.0] * 5
        assert made[14].shape == (4, 3)
        leaf = torch.zeros(6, 3, device=device, requires_grad=True)
        assert leaf.requires_grad and leaf.is_leaf and leaf.data_ptr() % 256 == 0
        (leaf * 2.0).sum().backward()
        assert float(leaf.grad.sum()) == 36.0
        leaf2 = torch.empty_like(src, requires_grad=True)
        assert leaf2.requires_grad and leaf2.is_leaf
        # copies that make a new tensor on the device are guarded; no-ops and differentiable copies are left alone
        n = len(g.allocations)
        host = torch.arange(6, dtype=torch.float32)
        moved = host.to(device) if torch.device(device).type != "cpu" else host.clone()
        cloned, packed = src.clone(), src.t().contiguous()
        assert len(g.allocations) == n + 3 and all(t.data_ptr() % 256 == 0 for t in (moved, cloned, packed))
        assert torch.equal(cloned, src) and torch.equal(packed, src.t()) and moved.tolist() == [0.0, 1.0, 2.0, 3.0, 4.0, 5.0]
        assert src.to(src.device) is src and src.contiguous() is src and len(g.allocations) == n + 3
        assert leaf.clone().grad_fn is not None and len(g.allocations) == n + 3


def check_poison_modes(device):
    with G.guarded_allocations(device, poison="float_nan") as g:
        f, i, z = torch.empty(33, device=device), torch.empty(33, dtype=torch.int32, device=device), torch.zeros(5, device=device)
        assert bool(torch.isnan(f).all()) and float(z.abs().sum()) == 0
        assert [al.fill for al in g.allocations] == ["nan", None, "value"]
    if torch.device(device).type != "cpu":
        return
    for byte in (0xFF, 0x5A):
        with G.guarded_allocations(device, poison="bytes", byte=byte) as g:
            f, i, o = torch.empty(33, device=device), torch.empty(33, dtype=torch.int32, device=device), torch.ones(5, device=device)
            assert bool((g.allocations[0].bytes() == byte).all()) and bool((g.allocations[1].bytes() == byte).all())
            assert int(i[0]) == (-1 if byte == 0xFF else 0x5A5A5A5A) and float(o.sum()) == 5.0
            assert [al.fill for al in g.allocations] == [byte, byte, "value"]


def check_pass_through(device):
    other = "cpu" if torch.device(device).type != "cpu" else "meta"
    with G.guarded_allocations(device) as g:
        a = torch.empty(10, device=other)
        b = torch.zeros(10, device=other)
        n = len(g.allocations)
        assert n == 0 and a.device.type == other and b.device.type == other
        if torch.cuda.is_available():
            q = torch.empty(4, pin_memory=True)
            assert q.is_pinned() and len(g.allocations) == n, "a pinned allocation was served from a guarded base"
        if torch.device(device).type != "cpu":          # (on the host build the pageable source of pin_memory() is itself a guarded host tensor)
            p = torch.zeros(2, dtype=torch.int32).pin_memory()
            assert p.is_pinned() and len(g.allocations) == n, "a pinned allocation was served from a guarded base"


def check_patches_are_put_back(device):
    methods = G._TENSOR_FACTORIES + G._TENSOR_COPIES
    before = [getattr(torch, n) for n in G._MODULE_FACTORIES] + [getattr(torch.Tensor, n) for n in methods]
    own = [n in torch.Tensor.__dict__ for n in methods]
    try:
        with G.guarded_allocations(device):
            patched = [getattr(torch, n) for n in G._MODULE_FACTORIES] + [getattr(torch.Tensor, n) for n in methods]
            assert all(a is not b for a, b in zip(before, patched))
            raise KeyError("leave through an exception")
    except KeyError:
        pass
    after = [getattr(torch, n) for n in G._MODULE_FACTORIES] + [getattr(torch.Tensor, n) for n in methods]
    assert all(a is b or a == b for a, b in zip(before, after))
    assert own == [n in torch.Tensor.__dict__ for n in methods]
    t = torch.arange(3)
    assert t.to(t.device) is t and t.clone().tolist() == [0, 1, 2]


def check_unchanged_helper(device):
    x = torch.tensor([1.0, float("nan"), 3.0], device=device)
    y = torch.arange(5, device=device)
    with G.unchanged(dict(x=x, y=y, absent=None, empty=torch.zeros(0, device=device))):
        x.clone().add_(1)                               # NaN stays NaN: equal bytes
    def write():
        with G.unchanged(dict(x=x, y=y)):
            y[3] = 9
    _raises(write, "const input y was written")


def check_find_and_records(device):
    with G.guarded_allocations(device) as g:
        a = torch.empty(300, dtype=torch.uint8, device=device)
        b = torch.empty(75, dtype=torch.float32, device=device)
        torch.empty(301, dtype=torch.uint8, device=device)
        assert [al.tensor.data_ptr() for al in g.find(300)] == [a.data_ptr(), b.data_ptr()]
        assert [al.tensor.data_ptr() for al in g.find(300, torch.uint8)] == [a.data_ptr()]
        rec = g.records()
        assert len(rec) == 3 and rec[0][1:] == (torch.uint8, (300,), 300, None) and "guard_selftest.py" in rec[0][0]
        assert g.owner(b.view(-1)[:10]) is g.allocations[1]
