"""Batched detection pipeline: the generalisation of test.py:do_test (test.py:121-161) from
one image per step to a whole batch with every stage on the device.

  images [B,3,S,S] -> RFBNet engine (fused HIP convs) -> [Context-Transformer attention]
  -> fused eval-softmax + decode + score fusion + `boxes *= scale`
  -> per (image, class): score > 0.01, descending-score order, NMS 0.45
  -> per image: keep score >= 200-th largest
  [-> box voting: every kept box becomes the score-weighted mean of the candidates of its class that overlap it]
With tta='hflip' the network also runs on the batch mirrored along W; that pass's boxes are mirrored back in pixels and both
candidate sets are pooled per image (2P rows) in front of the post-processing.
Results equal the reference's sequential per-image / per-class loop on the same
(loc, conf, obj): all_boxes[img][cls] = float32 [k,5] rows in descending score order.

The whole step (about 100 launches on two streams) allocates nothing and never synchronises with the host, so
after two eager steps it is captured once into a hipGraph and replayed (CTDET_GRAPH=0 keeps eager launches): at
small batches the step is otherwise bound by the host issuing launches, not by the GPU.  Weight re-packing
(parameter updates) stays outside the graph: it rewrites the same packed buffers the captured launches read.
"""
import os
import warnings

import torch

from . import ops


class DetectionPipeline:
    tta, passes, box_vote = None, 1, None           # the defaults: one pass, no voting

    def __init__(self, net, priors, batch, num_fg, image_wh=(500, 375), conf_thresh=0.01, nms_thresh=0.45,
                 max_per_image=200, force_cpu_rule=False, variance=(0.1, 0.2), out_cap=None, graph=None,
                 nms_method='hard', soft_sigma=0.5, soft_score_threshold=0.001, tta=None, box_vote=None,
                 matrix_pre_top=1024):
        """nms_method 'hard' (default), 'linear' or 'gaussian': the last two run soft-NMS (cpu_soft_nms methods 1 / 2,
        Nt = nms_thresh, sigma = soft_sigma, rows below soft_score_threshold dropped) in place of hard NMS.
        'matrix_linear' / 'matrix_gaussian': Matrix NMS (cpu_matrix_nms methods 1 / 2) on the best matrix_pre_top candidates
        of every class, sigma = soft_sigma, rows below soft_score_threshold dropped; nms_thresh does not apply.
        tta 'hflip': two passes, the second on the mirrored batch; self.boxes / self.scores are then the merged [B,2P,...]
        buffers (pass 0's P rows, then pass 1's mirrored back: x1' = W - x2, x2' = W - x1), the post-processor works on 2P
        rows and out_index holds merged indices k*P + p (pass k, prior p).
        box_vote (a float in (0, 1]): ops.box_vote with that IoU threshold after the top-k cut; may be changed between
        runs.  Both default to off, and the step then makes exactly the calls it makes without them."""
        self.net = net
        self.device = net._device()
        self.priors = priors.to(self.device, torch.float32).contiguous()
        self.batch, self.T = batch, num_fg
        self.P = self.priors.shape[0]
        self.variance = variance
        self.conf_thresh, self.nms_thresh, self.max_per_image = conf_thresh, nms_thresh, max_per_image
        self.ge = bool(force_cpu_rule)
        if ops.nms_method_number(nms_method)[0]:    # a misspelt method fails here, not in the first step
            ops.matrix_pre_top(matrix_pre_top)
        self.nms_method, self.soft_sigma, self.soft_score_threshold = nms_method, soft_sigma, soft_score_threshold
        self.matrix_pre_top = matrix_pre_top
        self.tta, self.passes = tta, ops.tta_mode(tta)
        ops.vote_threshold(box_vote)
        self.box_vote = box_vote
        self.scale = None
        self.set_image_wh(image_wh)
        self.rt = net.runtime(batch, self.device)
        rows = self.passes * self.P
        self.post = ops.PostProcessor(batch, rows, num_fg, self.device, out_cap)
        self.boxes = torch.empty(batch, rows, 4, device=self.device)
        self.scores = torch.empty(batch, rows, num_fg + 1, device=self.device)
        self.stage = self.x_flip = None
        if self.passes > 1:
            # one pass's ct_detect_fused output (both passes use it in turn) and the mirrored batch
            self.stage = (torch.empty(batch, self.P, 4, device=self.device),
                          torch.empty(batch, self.P, num_fg + 1, device=self.device))
            self.x_flip = torch.empty((batch,) + tuple(self.rt.plan.buf_shapes['x']), device=self.device)
        self.use_graph = (os.environ.get('CTDET_GRAPH', '1') != '0') if graph is None else bool(graph)
        if len(getattr(self.rt, 'sides', None) or []) > 1:
            # more than one side stream (CTDET_STREAMS > 2): ROCm 7.2 crashes in hipStreamEndCapture on that fork/join
            # pattern (measured); those schedules launch eagerly
            self.use_graph = False
        self._graph, self._eager_runs, self._graph_key = None, 0, None

    def set_image_wh(self, image_wh):
        """`scale` of test.py:122-123: one (w, h) for all images or one per image [B,2]."""
        wh = torch.as_tensor(image_wh, dtype=torch.float32)
        if wh.dim() == 1:
            new = torch.stack([wh[0], wh[1], wh[0], wh[1]])
        else:
            if wh.shape[0] != self.batch:
                raise ValueError('image_wh has %d rows, pipeline batch is %d' % (wh.shape[0], self.batch))
            new = torch.stack([wh[:, 0], wh[:, 1], wh[:, 0], wh[:, 1]], 1).contiguous()
        if self.scale is not None and self.scale.shape == new.shape:
            self.scale.copy_(new)                   # same buffer: a captured graph keeps reading it
        else:
            self.scale = new.to(self.device)
            self._graph = None

    def _net_key(self):
        """Everything a captured step froze besides the packed conv weights (which are rewritten in place): whether the
        Context-Transformer block runs, its 'incre' branch, the host-side value of `scale` and the raw pointers of the
        block's parameters -- a load_state_dict that changes `scale`, a re-allocated parameter (net.to(), assign=True)
        or a change of method / phase / setting re-captures instead of replaying stale arguments."""
        net = self.net
        key = (getattr(net, 'method', None), getattr(net, 'phase', None), getattr(net, 'setting', None))
        if key[0] == 'ours' and key[1] == 2:
            prm = net._ctx_params()
            key += tuple(v.data_ptr() if isinstance(v, torch.Tensor) else v for _, v in sorted(prm.items()))
        return key

    def _post_key(self):
        """The post-processing arguments a captured step froze."""
        key = (self.conf_thresh, self.nms_thresh, self.ge, self.max_per_image)
        if self._matrix():
            key += (self.nms_method, float(self.soft_sigma), float(self.soft_score_threshold), int(self._pre_top()))
        elif self.nms_method != 'hard':
            key += (ops.soft_method(self.nms_method), float(self.soft_sigma), float(self.soft_score_threshold))
        if self.tta is not None or self.box_vote is not None:
            key += (self.tta, ops.vote_threshold(self.box_vote))
        return key

    def _matrix(self):
        return ops.nms_method_number(self.nms_method)[0]

    def _pre_top(self):
        return getattr(self, 'matrix_pre_top', 1024)

    def _detect(self, out):
        """The network on rt.bufs['x'] and the fused decode into out = (boxes [B,P,4], scores [B,P,T+1])."""
        loc, conf, obj = self.net.forward_raw(None, _input_loaded=True, _batch=self.batch)
        ops.detect_fused(loc, conf.contiguous(), obj, self.priors, self.variance, True, self.scale, out=out)

    def _step(self):
        """The launches of one step on the current stream; reads rt.bufs['x'] (already filled) and, for the second
        pass of tta='hflip', self.x_flip."""
        merged = (self.boxes, self.scores)
        if self.passes == 1:
            self._detect(merged)
        else:
            self._detect(self.stage)
            ops.tta_merge(self.stage[0], self.stage[1], 0, self.passes, False, self.scale, merged)
            self.rt.copy_input(self.x_flip)
            self._detect(self.stage)
            ops.tta_merge(self.stage[0], self.stage[1], 1, self.passes, True, self.scale, merged)
        vote = () if self.box_vote is None else (self.box_vote,)
        if self._matrix():                          # (the other methods keep the call they had)
            vote = (self.box_vote, self._pre_top())
        self.post.run(self.boxes, self.scores, self.conf_thresh, self.nms_thresh, self.ge, self.max_per_image,
                      self.nms_method, self.soft_sigma, self.soft_score_threshold, *vote)

    def _capture(self):
        g = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(g):
                self._step()
        except Exception as e:                      # not a fallback to another device path: the same HIP launches, eagerly
            warnings.warn('hipGraph capture of the detection step failed (%s: %s); launching eagerly'
                          % (type(e).__name__, e))
            self.use_graph = False
            torch.cuda.synchronize(self.device)
            return None
        return g

    @torch.no_grad()
    def run(self, x, image_wh=None):
        """x [B,3,S,S] (device) -> (out_dets [B,T,cap,5], out_count [B,T]) device tensors."""
        if self.net.training:
            raise RuntimeError('DetectionPipeline runs the eval-mode network (call net.eval() first)')
        if image_wh is not None:
            self.set_image_wh(image_wh)
        rt = self.rt
        rt.load_input(x)                            # shape check, weight refresh, copy into the plan's input buffer
        if self.passes > 1:
            ops.hflip(x, out=self.x_flip)           # reads the caller's tensor: outside the captured step, like the copy above
        if hasattr(rt, 'ensure_wired'):
            rt.ensure_wired()
        be = rt.backend
        # (kernel_epoch: a step changed kernels; ws_generation: a three-kernel-Winograd workspace was re-allocated -- either way
        # a captured graph holds stale launches / pointers)
        key = self._post_key() + (rt.event_log is None, getattr(be, 'kernel_epoch', 0),
                                  getattr(be, 'ws_generation', 0)) + self._net_key()
        if self.use_graph and rt.event_log is None:
            if self._graph is not None and self._graph_key == key:
                self._graph.replay()
                return self.post.out_dets, self.post.out_count
            if self._eager_runs >= 2:               # lazily initialised state (function attributes, autotune) is settled
                self._graph = self._capture()
                self._graph_key = key
                if self._graph is not None:
                    self._graph.replay()
                    return self.post.out_dets, self.post.out_count
        self._eager_runs += 1
        self._step()
        return self.post.out_dets, self.post.out_count

    def results(self):
        """Host copy in the reference's all_boxes layout (synchronises)."""
        return self.post.to_all_boxes()
