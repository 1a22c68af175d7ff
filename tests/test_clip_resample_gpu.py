"""GPU: vj_clip_resample (jepa_amd/csrc/image_resample.hip) byte for byte against Pillow's Image.resize on every case of
tests/golden/frame_folder_micro.npz, for both filters: landscape, portrait, an upscale whose rows are 63 bytes long, a reduction by
4.04 (11 taps), a square and a native clip.  Integer arithmetic on both sides, so the comparison is np.array_equal throughout."""
import numpy as np
import pytest
import torch

from jepa_amd.app.vjepa.transforms import pack_buffers, resample_taps
from tests.frame_folder_util import case, centre_names, view_names

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD, FILL = 64, 0xA5
FILTERS = (("bilinear", 0, 1.0), ("bicubic", 1, 2.0))
NAMES = view_names() + centre_names()


def _two_frames(c, key):
    """Two frames of a case (its first one twice where it has one), so that clips of every case fit one launch."""
    a = c[key]
    return a[[0, min(1, len(a) - 1)]]


def _plan(sources, sizes, support, T, gap=0):
    """desc, rgeom, desc_out (with `gap` bytes of padding after every clip), out bytes and capacities of a launch, on the host."""
    flat, offs = pack_buffers([torch.from_numpy(s) for s in sources])
    desc = torch.tensor([[o, s.shape[1], s.shape[2], 0] for o, s in zip(offs, sources)], dtype=torch.int64)
    rgeom = torch.tensor(sizes, dtype=torch.int32).reshape(len(sizes), 2)
    rows, at = [], 0
    for OH, OW in sizes:
        rows.append([at, OH, OW, 0])
        at += -(-(T * OH * OW * 3 + gap) // 16) * 16
    caps = (max(s[0] for s in sizes), max(s[1] for s in sizes),
            max(resample_taps(s.shape[2], z[1], support) for s, z in zip(sources, sizes)),
            max(resample_taps(s.shape[1], z[0], support) for s, z in zip(sources, sizes)), max(s.shape[1] for s in sources))
    return flat, desc, rgeom, torch.tensor(rows, dtype=torch.int64), at, caps


def _run(flat, desc, rgeom, desc_out, nbytes, caps, T, code):
    """The launch between guards: (out bytes as numpy, the whole guarded buffer as numpy)."""
    from jepa_amd.hip import ops
    buf = torch.full((GUARD + nbytes + GUARD,), FILL, dtype=torch.uint8, device=DEV)
    out = buf[GUARD:GUARD + nbytes]
    ops.clip_resample(flat.to(DEV), desc.to(DEV), rgeom.to(DEV), T, code, caps, out, desc_out.to(DEV))
    torch.cuda.synchronize()
    whole = buf.cpu().numpy()
    assert (whole[:GUARD] == FILL).all() and (whole[GUARD + nbytes:] == FILL).all(), "guard bytes were written"
    return whole[GUARD:GUARD + nbytes]


def _clip(out, row, T):
    off, OH, OW = (int(v) for v in row[:3])
    return out[off:off + T * OH * OW * 3].reshape(T, OH, OW, 3)


@pytest.mark.parametrize("filt", [f[0] for f in FILTERS])
@pytest.mark.parametrize("name", NAMES)
def test_one_clip_equals_pillow(name, filt):
    _, code, support = next(f for f in FILTERS if f[0] == filt)
    c = case(name)
    T, size = len(c["frames"]), tuple(int(v) for v in c["resize"])
    plan = _plan([c["frames"]], [size], support, T)
    out = _run(*plan, T, code)
    assert np.array_equal(_clip(out, plan[3][0], T), c[filt]), name
    if tuple(c["frames"].shape[1:3]) == size:
        assert np.array_equal(c[filt], c["frames"])          # a native clip comes out as it went in


@pytest.mark.parametrize("filt", [f[0] for f in FILTERS])
def test_all_clips_in_one_launch_with_padding_between_them(filt):
    _, code, support = next(f for f in FILTERS if f[0] == filt)
    cs = [case(n) for n in NAMES]
    sources, sizes = [_two_frames(c, "frames") for c in cs], [tuple(int(v) for v in c["resize"]) for c in cs]
    flat, desc, rgeom, desc_out, nbytes, caps = _plan(sources, sizes, support, 2, gap=40)
    assert any(s.shape[1:3] == z for s, z in zip(sources, sizes)) and len({z for z in sizes}) > 3
    out = _run(flat, desc, rgeom, desc_out, nbytes, caps, 2, code)
    written = np.zeros(nbytes, dtype=bool)
    for n, c, row in zip(NAMES, cs, desc_out):
        assert np.array_equal(_clip(out, row, 2), _two_frames(c, filt)), n
        written[int(row[0]):int(row[0]) + 2 * int(row[1]) * int(row[2]) * 3] = True
    assert (~written).sum() >= 40 * len(cs) and (out[~written] == FILL).all(), "padding between clips was written"


def test_a_row_whose_source_or_destination_leaves_its_buffer_becomes_zeros_and_its_neighbours_are_exact():
    names = ["views_landscape", "views_upscale", "views_portrait"]
    cs = [case(n) for n in names]
    sources, sizes = [_two_frames(c, "frames") for c in cs], [tuple(int(v) for v in c["resize"]) for c in cs]
    flat, desc, rgeom, desc_out, nbytes, caps = _plan(sources, sizes, 1.0, 2, gap=40)

    def check(out, dout, zeroed):
        for k, (c, row) in enumerate(zip(cs, dout)):
            off, n = int(row[0]), 2 * int(row[1]) * int(row[2]) * 3
            if k == zeroed:
                assert (out[off:min(off + n, nbytes)] == 0).all(), names[k]
            else:
                assert np.array_equal(_clip(out, row, 2), _two_frames(c, "bilinear")), names[k]

    # the source of the middle clip is said to be taller than the frame buffer holds
    bad = desc.clone()
    bad[1, 1] = 1 + flat.numel() // (2 * int(desc[1, 2]) * 3)
    check(_run(flat, bad, rgeom, desc_out, nbytes, (caps[0], caps[1], caps[2], caps[3], int(bad[1, 1])), 2, 0), desc_out, 1)
    # a negative source offset
    bad = desc.clone()
    bad[0, 0] = -16
    check(_run(flat, bad, rgeom, desc_out, nbytes, caps, 2, 0), desc_out, 0)
    # the destination of the last clip ends 32 bytes behind `out`: zeros up to the end of out, nothing behind it (_run's guards)
    short = nbytes - 40 - 32
    short -= short % 16
    assert int(desc_out[2, 0]) + 2 * sizes[2][0] * sizes[2][1] * 3 > short > int(desc_out[2, 0])
    check(_run(flat, desc, rgeom, desc_out, short, caps, 2, 0)[:short], desc_out, 2)
    # a vertical tap capacity that only the upscale fits: the two reductions are zeroed
    tight = (caps[0], caps[1], caps[2], 3, caps[4])
    out = _run(flat, desc, rgeom, desc_out, nbytes, tight, 2, 0)
    assert resample_taps(37, 26) > 3 and resample_taps(23, 16) > 3 and resample_taps(11, 16) == 3
    for k, (c, row) in enumerate(zip(cs, desc_out)):
        got = _clip(out, row, 2)
        assert np.array_equal(got, _two_frames(c, "bilinear")) if k == 1 else not got.any(), names[k]


def test_an_empty_batch_launches_nothing_and_bad_arguments_are_refused_on_the_host():
    from jepa_amd.hip import ops
    from jepa_amd.hip.lib import HipKernelError
    out = torch.full((64,), FILL, dtype=torch.uint8, device=DEV)
    z64, z32 = torch.zeros((0, 4), dtype=torch.int64, device=DEV), torch.zeros((0, 2), dtype=torch.int32, device=DEV)
    ops.clip_resample(torch.zeros(16, dtype=torch.uint8, device=DEV), z64, z32, 2, 0, (1, 1, 3, 3, 1), out, z64)
    torch.cuda.synchronize()
    assert (out.cpu() == FILL).all()
    c = case("views_landscape")
    flat, desc, rgeom, desc_out, nbytes, caps = _plan([c["frames"]], [(16, 28)], 1.0, 3)
    args = (flat.to(DEV), desc.to(DEV), rgeom.to(DEV))
    big = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="filter"):
        ops.clip_resample(*args, 3, 2, caps, big, desc_out.to(DEV))
    with pytest.raises(ValueError, match="bad dims"):
        ops.clip_resample(*args, 3, 0, (16, 1 << 15, 5, 5, 23), big, desc_out.to(DEV))
    with pytest.raises(ValueError, match="needed"):
        ops.clip_resample(*args, 3, 0, caps, big, desc_out.to(DEV), ws=torch.zeros(16, dtype=torch.uint8, device=DEV))
    with pytest.raises(HipKernelError, match="aligned"):
        ops.clip_resample(*args, 3, 0, caps, torch.zeros(nbytes + 16, dtype=torch.uint8, device=DEV)[4:], desc_out.to(DEV))
