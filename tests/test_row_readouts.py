"""What the read-outs with a workspace of the caller's share (outline, texture, match, centreline, lobes), tested once for the five:
the workspace classes on _workspace.Workspace (CPU: the size query needs no device and the buffer may be host memory), and the -1 fill of
an int8 plane that the centreline and the lobe read-out launch (contact_rows.hpp) at its smallest shapes (GPU).
"""
import numpy as np
import pytest

# (module, class, sizes (h, w, batch, max_contacts, *more), names of what follows batch): the sizes are the smallest every read-out takes
WORKSPACES = {
    "outline": ("outline", "OutlineWorkspace", (24, 32, 3, 5), ("max_contacts",)),
    "texture": ("texture", "TextureWorkspace", (24, 32, 3, 5, 4), ("max_contacts", "max_lag")),
    "match": ("match", "MatchWorkspace", (24, 32, 3, 5, 9, 2, 19), ("max_contacts", "P", "max_shift", "M")),
    "centreline": ("centreline", "CentrelineWorkspace", (24, 32, 3, 5), ("max_contacts",)),
    "lobes": ("lobes", "LobesWorkspace", (24, 32, 3, 5), ("max_contacts",)),
}


@pytest.mark.parametrize("name", sorted(WORKSPACES))
def test_workspace_is_sized_aligned_and_fits_its_own_sizes_only(pkg, name):
    mod, cls, sizes, more = WORKSPACES[name]
    mod = getattr(pkg, mod)
    ws = getattr(mod, cls)(*sizes, device="cpu")
    assert ws.nbytes == mod.workspace_bytes(*sizes) > 0
    first, end = ws.buffer.data_ptr(), ws.buffer.data_ptr() + ws.buffer.numel()
    assert ws.pointer() % 256 == 0 and first <= ws.pointer() and ws.pointer() + ws.nbytes <= end
    batch = sizes[2]
    assert all(ws.fits(*sizes[:2], b, *sizes[3:]) for b in range(1, batch + 1))
    assert not ws.fits(*sizes[:2], batch + 1, *sizes[3:])
    for i, what in [(0, "h"), (1, "w")] + [(3 + j, n) for j, n in enumerate(more)]:
        other = list(sizes)
        other[i] += 1
        assert not ws.fits(*other), what
    ws.close()
    assert ws.buffer is None and not ws.fits(*sizes)


SENTINEL = 77
# below one block of the fill, exactly its 4 096 elements, one over, two frames ending mid-block
FILL_SHAPES = [(1, 1, 1), (1, 3, 5), (1, 64, 64), (1, 64, 65), (2, 65, 63)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", FILL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fill_writes_every_byte_of_the_plane_of_frames_without_contacts(pkg, shape):
    """vistaf_lobes_measure with d_lobe_index and vistaf_centreline_measure with d_skeleton, as contact_lobes(lobe_index=True) and
    contact_centrelines(skeleton=True) call them, on frames whose count is 0: the planes, filled with a sentinel first (which the wrappers'
    own torch.empty cannot be), are -1 in every byte and every row of the tables is NaN."""
    import torch
    B, h, w = shape
    K, L = 2, 3
    dev = torch.device("cuda:0")
    idx = torch.zeros((B, h, w), dtype=torch.int8, device=dev)
    tab = torch.full((B, K, 16), float("nan"), dtype=torch.float64, device=dev)
    cnt, mpp = torch.zeros((B,), dtype=torch.int32, device=dev), torch.full((B,), 0.1, dtype=torch.float64, device=dev)
    dep = torch.ones((B, h, w), dtype=torch.float32, device=dev)

    def workspace(mod):
        n = mod.workspace_bytes(h, w, B, K)
        buf = torch.empty((n + 256,), dtype=torch.uint8, device=dev)
        return buf, (buf.data_ptr() + 255) & ~255, n
    lobes = torch.full((B, K, L, 16), 123.0, dtype=torch.float64, device=dev)
    rows = torch.full((B, K, 12), 123.0, dtype=torch.float64, device=dev)
    lidx = torch.full((B, h, w), SENTINEL, dtype=torch.int8, device=dev)
    keep, p, n = workspace(pkg.lobes)
    pkg._handle.call(dev, "vistaf_lobes_measure", idx.data_ptr(), tab.data_ptr(), cnt.data_ptr(), mpp.data_ptr(), dep.data_ptr(), B, h, w, K, L, 0.02, 0.1,
                     0.0, lobes.data_ptr(), rows.data_ptr(), lidx.data_ptr(), None, None, None, None, p, n, pkg._handle.stream(dev))
    out = torch.full((B, K, 40), 123.0, dtype=torch.float64, device=dev)
    sk = torch.full((B, h, w), SENTINEL, dtype=torch.int8, device=dev)
    keep2, p, n = workspace(pkg.centreline)
    pkg._handle.call(dev, "vistaf_centreline_measure", idx.data_ptr(), tab.data_ptr(), cnt.data_ptr(), mpp.data_ptr(), None, B, h, w, K, 8, 0, out.data_ptr(),
                     None, None, None, sk.data_ptr(), p, n, pkg._handle.stream(dev))
    torch.cuda.synchronize()
    assert (lidx.cpu().numpy() == -1).all() and (sk.cpu().numpy() == -1).all()
    assert np.isnan(lobes.cpu().numpy()).all() and np.isnan(rows.cpu().numpy()).all() and np.isnan(out.cpu().numpy()).all()
