"""Winograd F(2x2,3x3) in plain torch (Lavin & Gray 2015): the specification of csrc/winograd.h and of forward_pm.wino_filter, in the
layouts the kernels use.  x [B,H,W,C] -> V [16,T,C]; g [O,C,3,3] -> U [16,O,C]; M [16,T,O] -> Y [B,H,W,O]; plane xi = 4u + v is
position (u, v) of the transformed 4 x 4 tile, tiles are numbered (b, ty, tx) with T = B * ceil(H/2) * ceil(W/2)."""
import torch
import torch.nn.functional as F

BT = [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]]
G = [[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]]
AT = [[1, 1, 1, 0], [0, 1, -1, -1]]


def tiles(B, H, W):
    return B * ((H + 1) // 2) * ((W + 1) // 2)


def input_transform(x):
    """V = B^T d B of the 4 x 4 windows at (2ty - 1, 2tx - 1), zeros outside the map"""
    B, H, W, C = x.shape
    H2, W2 = (H + 1) // 2 * 2, (W + 1) // 2 * 2
    xp = F.pad(x.permute(0, 3, 1, 2), (1, 1 + W2 - W, 1, 1 + H2 - H))
    d = xp.unfold(2, 4, 2).unfold(3, 4, 2)                                # [B,C,th,tw,4,4]
    bt = torch.tensor(BT, dtype=x.dtype, device=x.device)
    v = bt @ d @ bt.T
    return v.permute(4, 5, 0, 2, 3, 1).reshape(16, -1, C)


def filter_transform(g, dtype=None):
    """U = G g G^T in float64, rounded once to `dtype` (default: the filter's)"""
    gm = torch.tensor(G, dtype=torch.float64, device=g.device)
    u = gm @ g.double() @ gm.T                                            # [O,C,4,4]
    return u.permute(2, 3, 0, 1).reshape(16, g.shape[0], g.shape[1]).to(dtype or g.dtype).contiguous()


def output_transform(m, shape):
    """Y = A^T m A, the 2 x 2 tiles laid back on the [B,H,W] map (cropped where H or W is odd)"""
    B, H, W = shape
    th, tw, O = (H + 1) // 2, (W + 1) // 2, m.shape[-1]
    at = torch.tensor(AT, dtype=m.dtype, device=m.device)
    mm = m.reshape(4, 4, B, th, tw, O).permute(2, 3, 4, 5, 0, 1)          # [B,th,tw,O,4,4]
    y = at @ mm @ at.T                                                    # [B,th,tw,O,2,2]
    return y.permute(0, 1, 4, 2, 5, 3).reshape(B, 2 * th, 2 * tw, O)[:, :H, :W].contiguous()


def conv(x, g):
    """3 x 3 convolution, stride 1, padding 1, of x [B,H,W,C] with g [O,C,3,3] -> [B,H,W,O]"""
    v, u = input_transform(x), filter_transform(g, x.dtype)
    return output_transform(torch.einsum("xtc,xoc->xto", v, u), x.shape[:3])
