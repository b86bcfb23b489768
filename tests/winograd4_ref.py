"""Winograd F(4x4,3x3) on the interpolation points 0, 1, -1, 2, -1/2 in plain torch: the specification of the F(4x4) kernels of
csrc/winograd.h and of forward_pm.wino4_filter, in the layouts the kernels use.  x [B,H,W,C] -> V [36,T,C]; g [O,C,3,3] -> U [36,O,C];
M [36,T,O] -> Y [B,H,W,O]; plane xi = 6u + v is position (u, v) of the transformed 6 x 6 tile, tiles are numbered (b, ty, tx) with
T = B * ceil(H/4) * ceil(W/4).  The rows of B^T are scaled to integers, the inverse scale is folded into G."""
import torch
import torch.nn.functional as F

BT = [[2, 3, -4, -3, 2, 0], [0, -2, -5, -1, 2, 0], [0, 2, 1, -5, 2, 0], [0, -1, -2, 1, 2, 0], [0, 2, -1, -2, 1, 0], [0, 2, 3, -4, -3, 2]]
G = [[1 / 2, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [1 / 6, -1 / 6, 1 / 6], [1 / 30, 1 / 15, 2 / 15], [-16 / 15, 8 / 15, -4 / 15], [0, 0, 1 / 2]]
AT = [[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -1 / 2, 0], [0, 1, 1, 4, 1 / 4, 0], [0, 1, -1, 8, -1 / 8, 1]]


def tiles(B, H, W):
    return B * ((H + 3) // 4) * ((W + 3) // 4)


def input_transform(x, bt=BT):
    """V = B^T d B of the 6 x 6 windows at (4ty - 1, 4tx - 1), zeros outside the map"""
    B, H, W, C = x.shape
    H4, W4 = (H + 3) // 4 * 4, (W + 3) // 4 * 4
    xp = F.pad(x.permute(0, 3, 1, 2), (1, 1 + W4 - W, 1, 1 + H4 - H))
    d = xp.unfold(2, 6, 4).unfold(3, 6, 4)                                # [B,C,th,tw,6,6]
    bt = torch.tensor(bt, dtype=x.dtype, device=x.device)
    v = bt @ d @ bt.T
    return v.permute(4, 5, 0, 2, 3, 1).reshape(36, -1, C)


def filter_transform(g, dtype=None, gm=G):
    """U = G g G^T in float64, rounded once to `dtype` (default: the filter's)"""
    gm = torch.tensor(gm, dtype=torch.float64, device=g.device)
    u = gm @ g.double() @ gm.T                                            # [O,C,6,6]
    return u.permute(2, 3, 0, 1).reshape(36, g.shape[0], g.shape[1]).to(dtype or g.dtype).contiguous()


def output_transform(m, shape, at=AT):
    """Y = A^T m A, the 4 x 4 tiles laid back on the [B,H,W] map (cropped where H or W is no multiple of 4)"""
    B, H, W = shape
    th, tw, O = (H + 3) // 4, (W + 3) // 4, m.shape[-1]
    at = torch.tensor(at, dtype=m.dtype, device=m.device)
    mm = m.reshape(6, 6, B, th, tw, O).permute(2, 3, 4, 5, 0, 1)          # [B,th,tw,O,6,6]
    y = at @ mm @ at.T                                                    # [B,th,tw,O,4,4]
    return y.permute(0, 1, 4, 2, 5, 3).reshape(B, 4 * th, 4 * tw, O)[:, :H, :W].contiguous()


def conv(x, g, mats=(BT, G, AT)):
    """3 x 3 convolution, stride 1, padding 1, of x [B,H,W,C] with g [O,C,3,3] -> [B,H,W,O]"""
    v, u = input_transform(x, mats[0]), filter_transform(g, x.dtype, mats[1])
    return output_transform(torch.einsum("xtc,xoc->xto", v, u), x.shape[:3], mats[2])
