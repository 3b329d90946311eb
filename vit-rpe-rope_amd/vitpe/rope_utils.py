"""Drop-in mirror of the reference's models/rope_utils.py on the HIP rotary kernel."""
import torch

from . import kernels as K


def reshape_for_broadcast(x, target_tensor):
    """[N,D/2] -> [1,1,N,D/2]; [H,N,D/2] -> [1,H,N,D/2]; else ValueError (reference rope_utils.py:39-65)."""
    if x.ndim == 3 and target_tensor.ndim == 4:
        return x.unsqueeze(0)
    elif x.ndim == 2 and target_tensor.ndim == 4:
        return x.unsqueeze(0).unsqueeze(0)
    else:
        raise ValueError(f"Unexpected tensor shapes: {x.shape} vs {target_tensor.shape}")


class _RotaryEmb(torch.autograd.Function):
    """Rotate-half of q and k under autograd: gradients w.r.t. q, k and (as independent inputs, like the reference's
    autograd) cos and sin, each only when it is asked for.  All on the HIP kernels (vitpe_apply_rotary[_bwd])."""

    @staticmethod
    def forward(ctx, q, k, cos, sin):
        ctx.meta = (q.dtype, k.dtype, cos.shape, cos.dtype, sin.shape, sin.dtype)
        while cos.ndim > 2 and cos.shape[0] == 1:
            cos, sin = cos.squeeze(0), sin.squeeze(0)
        cos, sin = cos.contiguous().float(), sin.contiguous().float()
        qf, kf = q.contiguous().float(), k.contiguous().float()
        tables = ctx.needs_input_grad[2] or ctx.needs_input_grad[3]
        # (the rotated inputs enter only the table gradients)
        ctx.save_for_backward(cos, sin, qf if tables else None, kf if tables else None)
        return K.apply_rotary(qf, cos, sin).to(q.dtype), K.apply_rotary(kf, cos, sin).to(k.dtype)

    @staticmethod
    def backward(ctx, dqr, dkr):
        cos, sin, qf, kf = ctx.saved_tensors
        qdt, kdt, cshape, cdt, sshape, sdt = ctx.meta
        need_q, need_k, need_c, need_s = ctx.needs_input_grad
        dcos = torch.zeros_like(cos) if need_c else None
        dsin = torch.zeros_like(sin) if need_s else None
        tables = need_c or need_s

        def one(dy, x, need_x, dt):
            if dy is None or not (need_x or tables):
                return None
            dyf = dy.contiguous().float()
            dx = K.apply_rotary_bwd(dyf, x if tables else dyf, cos, sin, dcos, dsin, want_dx=need_x)
            return dx.to(dt) if need_x else None

        dq = one(dqr, qf, need_q, qdt)   # q and k accumulate into the same dcos / dsin
        dk = one(dkr, kf, need_k, kdt)
        return (dq, dk, dcos.view(cshape).to(cdt) if need_c else None, dsin.view(sshape).to(sdt) if need_s else None)


def apply_rotary_emb(q, k, cos, sin):
    """Rotate-half RoPE on q,k [B,H,N,D] with pairs (j, j+D/2) (reference rope_utils.py:3-37).
    cos/sin as produced by reshape_for_broadcast ([1,1,N,D/2] or [1,H,N,D/2]) or un-reshaped.
    Differentiable w.r.t. q, k, cos and sin (cos and sin as independent inputs); dq / dk in the dtype of q / k, dcos /
    dsin in the shape the caller passed."""
    return _RotaryEmb.apply(q, k, cos, sin)
