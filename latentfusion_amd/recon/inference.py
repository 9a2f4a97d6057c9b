"""LatentFusionModel: the inference facade the pose estimators drive (API mirror of
latentfusion/recon/inference.py:14-149)."""
from pathlib import Path

import torch

from ..observation import KERNELS as PREPROCESS_KERNELS
from ..observation import Observation, fused_preprocess
from . import models


class _Frozen:
    def __init__(self, model):
        self.params = None
        self.model = model

    def __enter__(self):
        self.params = [p for p in self.model.parameters() if p.requires_grad]
        for p in self.params:
            p.requires_grad_(False)
        return self.model

    def __exit__(self, *exc):
        for p in self.params:
            p.requires_grad_(True)
        return False


class LatentFusionModel:
    preprocess_kernel = 'composed'      # (also what an instance made without __init__ runs)

    @classmethod
    def from_checkpoint(cls, checkpoint, device='cpu', ibr_kernel=None, preprocess_kernel='composed'):
        if isinstance(checkpoint, (Path, str)):
            checkpoint = torch.load(checkpoint, map_location='cpu', weights_only=False)
        sculptor, fuser, photographer, _, generator = models.load_models(checkpoint, device=device, return_generator=True)
        return cls(sculptor, fuser, photographer, checkpoint['args']['camera_dist'], device, generator=generator,
                   ibr_kernel=ibr_kernel, preprocess_kernel=preprocess_kernel)

    def __init__(self, sculptor, fuser, photographer, camera_dist, device, generator=None, ibr_kernel=None,
                 preprocess_kernel='composed'):
        """ibr_kernel: how the colour paths reproject (ibr.reproject_views): None = ibr.KERNEL, 'composed' or 'fused'.
        preprocess_kernel: how preprocess_observation runs: 'composed' (zoom, prepare, normalize step by step) or 'fused' (one
        ops.observation_prepare call for a device observation none of whose meta flags is set; anything else stays composed)."""
        if preprocess_kernel not in PREPROCESS_KERNELS:
            raise ValueError(f'preprocess_kernel {preprocess_kernel!r}: one of {PREPROCESS_KERNELS}')
        self.device = device
        self.ibr_kernel = ibr_kernel
        self.preprocess_kernel = preprocess_kernel
        self.sculptor, self.fuser, self.photographer = sculptor.to(device), fuser.to(device), photographer.to(device)
        self.generator = generator.to(device) if generator is not None else None
        self.camera_dist = camera_dist
        self.input_size = sculptor.in_size
        self.eval()

    def eval(self):
        return self.train(False)

    def train(self, train=True):
        """Switches the modules' train / eval mode, like the reference (recon/inference.py:39-49).  Whether parameters
        take gradients is a separate matter: see freeze() / frozen()."""
        for m in self._modules():
            m.train(train)
        return self

    def _modules(self):
        return [m for m in (self.sculptor, self.photographer, self.fuser, self.generator) if m is not None]

    def parameters(self):
        for m in self._modules():
            yield from m.parameters()

    def freeze(self):
        """requires_grad False on every parameter: no weight-gradient kernel is launched by a backward through this
        model (the reference's pose loops accumulate weight gradients nobody reads)."""
        for p in self.parameters():
            p.requires_grad_(False)
        return self

    def unfreeze(self):
        for p in self.parameters():
            p.requires_grad_(True)
        return self

    def frozen(self):
        """Context manager: parameters frozen inside, every parameter's own flag restored on exit.  The pose
        estimators run under it, so a model that is also being trained keeps its flags."""
        return _Frozen(self)

    def zoom_observation(self, observation):
        if not observation.meta['is_zoomed']:
            return observation.zoom(self.camera_dist, self.input_size)
        return observation

    def _fused_applies(self, observation):
        """One fused call serves a device observation that is neither zoomed, prepared nor normalized."""
        meta = observation.meta
        return (self.preprocess_kernel == 'fused' and not (meta['is_zoomed'] or meta['is_prepared'] or meta['is_normalized'])
                and observation.depth.is_cuda)

    def preprocess_observation(self, observation):
        if self._fused_applies(observation):
            return fused_preprocess(observation, self.camera_dist, self.input_size, prepare=True, normalize=True)[0]
        if not observation.meta['is_zoomed']:
            observation = observation.zoom(self.camera_dist, self.input_size)
        if not observation.meta['is_prepared']:
            observation = observation.prepare()
        if not observation.meta['is_normalized']:
            observation = observation.normalize()
        return observation

    def build_latent_object(self, observation: Observation):
        """Reference views -> fused latent volume (1,1,C,S,S,S)."""
        observation = observation.to(self.device)
        x = None
        if self._fused_applies(observation) and self.sculptor.input_color and self.sculptor.input_mask:
            # the kernel also writes the encoder's stacked input: Sculptor.encode skips its concatenation
            stack = 'color_depth_mask' if self.sculptor.input_depth else 'color_mask'
            observation, x = fused_preprocess(observation, self.camera_dist, self.input_size, prepare=True, normalize=True,
                                              stack=stack)
        else:
            observation = self.preprocess_observation(observation)
        with torch.no_grad():
            z_obj, _ = self.sculptor.encode(self.fuser, camera=observation.camera, color=observation.color.unsqueeze(0),
                                            depth=observation.depth.unsqueeze(0), mask=observation.mask.unsqueeze(0), x=x)
        return z_obj

    def compute_latent_code(self, observation, camera):
        observation = self.preprocess_observation(observation)
        if len(observation) == 1:
            observation = observation.expand(len(camera))
        _, feats = models.autoencode(self.sculptor, self.fuser, self.photographer, camera=camera,
                                     color=observation.color.unsqueeze(1), depth=observation.depth.unsqueeze(1),
                                     mask=observation.mask.unsqueeze(1))
        return feats

    def render_latent_object(self, z_obj, camera, return_latent=True, apply_mask=True):
        y, z, _ = self.photographer.decode(z_obj, camera, return_latent=return_latent, apply_mask=apply_mask)
        if return_latent:
            z = z.squeeze(0)
        return y, z

    def render_ibr_basic(self, z_obj, input_obs, camera_out, return_latent=True, apply_mask=True, p=0.5):
        from .. import ibr
        from ..three.batchview import b2bv
        input_obs = self.preprocess_observation(input_obs)
        y, z = ibr.render_latent_ibr2(self.photographer, z_obj, input_obs.camera.clone().to(self.device),
                                      camera_out.clone().to(self.device),
                                      b2bv(input_obs.color, batch_size=1).to(self.device), p=p, weight_type='cam_dist',
                                      return_latent=return_latent, apply_mask=apply_mask, kernel=self.ibr_kernel)
        if return_latent:
            z = z.squeeze(0)
        return {k: v.squeeze(0) for k, v in y.items()}, z

    def render_ibr(self, z_obj, input_obs, camera_out, return_latent=True):
        """Colour by the learned IBR generator (reference recon/inference.py:151-191): the reprojected input views,
        their reprojected depths and a camera-similarity plane per view are stacked into the generator U-Net, whose
        logits blend the views per pixel after a residual flow of at most 5 pixels (ibr.warp_blend_logits)."""
        from .. import ibr
        if self.generator is None:
            raise ValueError('this checkpoint carries no IBR generator (modules.generator)')
        input_obs = self.preprocess_observation(input_obs)
        stack = None
        if ibr._resolve_kernel(self.ibr_kernel) == 'fused':
            # the generator's stacked input (B*V_o, V_i, C+2, H, W): the fused kernel writes colour and depth straight into it
            v_i, c, h, w = input_obs.color.shape
            stack = torch.empty(len(camera_out), v_i, c + 2, h, w, device=input_obs.color.device, dtype=torch.float32)
        y_out, z_out, image_reproj, depth_reproj, _mask_out, depth_out, _dist_r, dist_t = self._render_reprojections(
            z_obj, input_obs.color, input_obs.camera, camera_out, out=stack)
        if return_latent:
            z_out = z_out.squeeze(0)
        sims = 1.0 - dist_t * 2
        if stack is not None and image_reproj.data_ptr() == stack.data_ptr():
            x = stack
            x[:, :, -1] = sims[:, :, None, None]
        else:
            x = torch.cat((image_reproj, depth_reproj,
                           sims[:, :, None, None, None].expand(-1, -1, -1, *image_reproj.shape[-2:])), dim=2)
        x = x.reshape(-1, x.shape[1] * x.shape[2], x.shape[3], x.shape[4])              # views folded into channels
        x = torch.cat((depth_out, x), dim=1)
        logits = self.generator(x)
        y_out['color'], _, _, _ = ibr.warp_blend_logits(logits, image_reproj, 5)
        return {k: v.squeeze(0) for k, v in y_out.items()}, z_out

    def _render_reprojections(self, z_obj, color_in, camera_in, camera_out, return_latent=True, out=None):
        """reference recon/inference.py:193-217: depths of the input and output views from the latent renderer, the
        input views reprojected into every output view and masked by the predicted output mask.  With the 'fused' IBR kernel
        the mask is applied in the kernel's store and, where nothing asks for a gradient, the results are written into `out`
        ((B*V_o, V_i, C+2, H, W), see ops.ibr_reproject) and returned as views of it."""
        from .. import ibr
        from ..three.batchview import bv2b
        y_in, _, _ = self.photographer.decode(z_obj, camera_in)
        y_out, z_out, _ = self.photographer.decode(z_obj, camera_out, return_latent=return_latent)
        mask_out, depth_out = y_out['mask'], y_out['depth']
        if ibr._resolve_kernel(self.ibr_kernel) == 'fused':
            color_in = color_in.unsqueeze(0)
            grad = torch.is_grad_enabled()
            in_kernel = not (grad and mask_out.requires_grad)                            # (the kernel's mask is a constant)
            if grad and any(t.requires_grad for t in (color_in, y_in['depth'], y_out['depth'])):
                out = None
            image_reproj, depth_reproj, dist_r, dist_t = ibr.reproject_views_batch(
                color_in, y_in['depth'], y_out['depth'], camera_in, camera_out, kernel='fused',
                mask_out=mask_out if in_kernel else None, out=out)
            if not in_kernel:
                image_reproj = image_reproj * mask_out.unsqueeze(2)
                depth_reproj = (depth_reproj + 1.0) * mask_out.unsqueeze(2) - 1.0
            return (y_out, z_out, bv2b(image_reproj), bv2b(depth_reproj), bv2b(mask_out), bv2b(depth_out), bv2b(dist_r),
                    bv2b(dist_t))
        image_reproj, depth_reproj, dist_r, dist_t = ibr.reproject_views_batch(color_in.unsqueeze(0), y_in['depth'],
                                                                                y_out['depth'], camera_in, camera_out,
                                                                                kernel='composed')
        image_reproj = image_reproj * mask_out.unsqueeze(2)
        depth_reproj = (depth_reproj + 1.0) * mask_out.unsqueeze(2) - 1.0
        return (y_out, z_out, bv2b(image_reproj), bv2b(depth_reproj), bv2b(mask_out), bv2b(depth_out), bv2b(dist_r),
                bv2b(dist_t))

    def render_full(self, z_obj, camera, input_obs=None, p=0.5):
        """Full-frame depth/mask(/colour).  Note SURVEY Q6: in the reference the input_obs=None branch
        raises (a 5-D tensor reaches uncrop); here that branch squeezes the object axis and works."""
        camera_zoom = camera.zoom(None, self.camera_dist, self.input_size).to(self.device)
        if input_obs is None:
            pred, _ = self.render_latent_object(z_obj, camera_zoom, apply_mask=True, return_latent=False)
            pred = {k: v.squeeze(0) for k, v in pred.items()}
        else:
            pred, _ = self.render_ibr_basic(z_obj, input_obs, camera_zoom, apply_mask=True, return_latent=False, p=p)
        out = {}
        mask = pred['mask']
        out['depth'], _ = camera_zoom.uncrop(camera_zoom.denormalize_depth(pred['depth']) * mask)
        out['mask'], _ = camera_zoom.uncrop(mask)
        if 'color' in pred:
            out['color'], _ = camera_zoom.uncrop(pred['color'] / 2 + 0.5)
        return out
