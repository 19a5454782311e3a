"""The predictor heads of the fused bf16 paths: conf and loc filters of a source map packed into one convolution, the launches that run
the packed heads of several maps at once, and the two-stream schedule that puts the trunk's heads beside the extra layers."""
import torch

from .. import _native as nat
from . import _conv_select as sel


class PredictorHeads:
    """The part of `SSDModel` (models/_common.py) that runs `conf_heads` / `loc_heads`; it uses the model's `_pick`, `_fused_train`,
    `_fused_head_ok`, `_conv_nobias` and `_packed_head_shadow`."""

    def _split_heads(self, x):
        """Fused bf16 inference only: the predictor heads of the trunk's two source maps (conv4_3, fc7: ~85 % of the head FLOPs) do not
        depend on the extra layers -- a chain of eight small convolutions that leaves most CUs idle -- so the two can share the chip
        on two HIP streams.  Mode 3 is what the HIP-graph step uses (GraphedInference; the eager path stays on one stream unless
        SSDHIP_HEAD_OVERLAP says otherwise): the two trunk heads as a grouped slab launch capped at 160 of the 256 CUs on the second
        stream beside the chain, then the four small heads (1.4 % / 0.7 % of a step in round 2; no measurable difference since the
        extra layers are split-K launches: profiles/r03zd_two_stream_heads_and_producer_priority_remeasured.txt).  Modes 1 | 2 are the older forms with the implicit-GEMM heads (1: the heads on the second stream; 2: the chain on
        a high-priority second stream): ~190 us of kernels run side by side but slow each other down by as much -- those heads fill
        every CU (r02p: 2.831 off / 2.832 / 2.815 ms).  Returns (feature maps, packed head outputs), or None for the one-stream path."""
        mode = sel.switch("HEAD_OVERLAP") or self.__dict__.get("_head_overlap") or "0"
        if (mode == "0" or not hasattr(self, "trunk_features") or not x.is_cuda
                or torch.is_grad_enabled() or not self.fused_inference or x.dtype != torch.bfloat16
                or len(self.conf_heads) > 8 + 2):
            return None
        if not all(conv.weight.dtype == torch.bfloat16 for conv in self.conf_heads):
            return None
        early = self.trunk_features(x)
        n_early = len(early)
        if not all(self._fused_head_ok(f, ch) and self._packed_head_ok(ch, lh, f)
                   for f, ch, lh in zip(early, self.conf_heads, self.loc_heads)):
            raise RuntimeError("predictor heads of the trunk do not qualify for the packed kernel")
        if mode in ("3", "4") and not self._halo_heads_ok(early):
            mode = "1"
        main = torch.cuda.current_stream(x.device)
        side = self.__dict__.get("_side_stream")
        if side is None or side.device != x.device:
            # An ORDINARY stream since round 6 (rounds 2-5: priority -1, "served first when both streams have workgroups pending" --
            # schedule 4 has no such moment: the capped launch leaves the chain its CUs).  Same box, 6 x 60 steps alternating: 2.0068 ms
            # (ordinary) vs 2.0072 ms (high priority); but once a process has USED a high-priority stream, every later HIP graph with
            # parallel branches replays slower on this runtime -- the reference-precision step 6.5 -> 7.6-7.9 ms, slower than its eager
            # form, which is what bench.py's second graph measured in rounds 5-6 (profiles/r06z_graphs_after_a_high_priority_stream.txt).
            side = torch.cuda.Stream(device=x.device, priority=int(sel.switch("SIDE_PRIORITY")))
            self.__dict__["_side_stream"] = side

        def check_rest(rest):
            if not all(self._fused_head_ok(f, ch) and self._packed_head_ok(ch, lh, f)
                       for f, ch, lh in zip(rest, self.conf_heads[n_early:], self.loc_heads[n_early:])):
                raise RuntimeError("predictor heads of the extra layers do not qualify for the packed kernel")

        # No record_stream anywhere: every tensor the other stream touches outlives the join in program order, and a block of the
        # side stream's pool is only reused after that stream has waited for the current one again.
        if mode == "4" and hasattr(self, "extra_features_front") and hasattr(self, "extra_features_tail"):
            # Round 4: the tail of the extra layers is ONE launch on one CU per image (csrc/ssdhip_chain.hip: 32 CUs, ~55 us), so the
            # balance moved: first the front of the extra layers (conv6_1, conv6_2: split-K launches that want the whole chip), THEN
            # the two trunk heads on the second stream capped so that one CU per image stays free, beside the tail and the small heads
            front = self.extra_features_front(early[1])
            # Round 6: conv6_2 exists BEFORE the fork, so its head rides in the capped launch with the two trunk heads instead of leading
            # the small launch behind the chain.  In units of 72 K-steps the capped launch is then 112 fc7 items x 2 + 192 conv4_3 items
            # + 32 conv6_2 items = 448 = exactly two per workgroup at 224 workgroups in the kernel's snake order (at 216 sixteen
            # workgroups draw an fc7 item AND a conv6_2 item: 132 us instead of 102), and 224 + the chain's 32 = the chip's 256 CUs.
            # Same box, alternating, 3 x 30 steps: 1.935 -> 1.926 ms per step (profiles/r06y_ab_head_split.txt).
            n_big = n_early + 1 if (sel.switch("HEAD_SPLIT") == "3" and self._halo_heads_ok([front])
                                    and self._fused_head_ok(front, self.conf_heads[n_early])
                                    and self._packed_head_ok(self.conf_heads[n_early], self.loc_heads[n_early], front)) else n_early
            big_maps = list(early) + ([front] if n_big > n_early else [])
            side.wait_stream(main)
            with torch.cuda.stream(side):
                big = nat.conv3x3_halo_group(big_maps, [self._packed_head_weight(l, 128) for l in range(n_big)], None, relu=False,
                                             max_workgroups=int(sel.switch("HEAD_WGS") or ("224" if n_big > n_early else "216")))
            rest = self.extra_features_tail(front)
            check_rest(rest)
            later = rest[n_big - n_early:]                    # the maps whose heads are still to come
            small = self._small_heads(later, n_big) if later else []
            main.wait_stream(side)
            return early + rest, big + small
        if mode in ("3", "4"):
            # the two trunk heads as a grouped slab launch capped at HALF the CUs (persistent workgroups, one per CU) on the second
            # stream, the latency-bound chain of extra layers on the current one in the other half, then the four small heads
            side.wait_stream(main)
            with torch.cuda.stream(side):
                big = nat.conv3x3_halo_group(list(early), [self._packed_head_weight(l, 128) for l in range(n_early)], None, relu=False,
                                             max_workgroups=int(sel.switch("HEAD_WGS") or "128"))
            rest = self.extra_features(early[1])
            check_rest(rest)
            small = self._small_heads(rest, n_early)
            main.wait_stream(side)
            return early + rest, big + small
        if mode == "2":
            # the latency-bound chain (extra layers + their small heads) on the high-priority stream, the two big heads on the current
            # one: the chain's few workgroups no longer queue behind ~600 head workgroups at every one of its eight launches
            side.wait_stream(main)
            with torch.cuda.stream(side):
                rest = self.extra_features(early[1])
                check_rest(rest)
                small = nat.conv2d_same_group(list(rest), [self._packed_head_weight(n_early + l) for l in range(len(rest))], None,
                                              relu=False)
            big = nat.conv2d_same_group(list(early), [self._packed_head_weight(l) for l in range(n_early)], None, relu=False)
            main.wait_stream(side)
            return early + rest, big + small
        side.wait_stream(main)
        with torch.cuda.stream(side):
            big = nat.conv2d_same_group(list(early), [self._packed_head_weight(l) for l in range(n_early)], None, relu=False)
        rest = self.extra_features(early[1])
        check_rest(rest)
        small = nat.conv2d_same_group(list(rest), [self._packed_head_weight(n_early + l) for l in range(len(rest))], None, relu=False)
        main.wait_stream(side)
        return early + rest, big + small

    def _small_heads(self, maps, first):
        """The packed heads of `maps` (predictor layers first, first + 1, ...) as one launch: the grouped slab launch, or the
        implicit-GEMM group for maps the slab kernel does not cover."""
        if self._halo_heads_ok(maps):
            return nat.conv3x3_halo_group(list(maps), [self._packed_head_weight(first + l, 128) for l in range(len(maps))], None, relu=False)
        return nat.conv2d_same_group(list(maps), [self._packed_head_weight(first + l) for l in range(len(maps))], None, relu=False)

    def _train_assembly_fits(self, n_maps):
        """The one-launch assembly backward runs for this model's packed heads (LDS need from libssdhip's own formula, cached)."""
        packs = [self._packed_head_shadow(l) for l in range(n_maps)]
        if any(pk is None for pk in packs):
            return False
        key = (self.n_classes, tuple(int(pb.n_boxes) for pb in self.priorboxes[:n_maps]), tuple(int(pk[0].shape[0]) for pk in packs))
        memo = self.__dict__.setdefault("_assembly_fits", {})
        if key not in memo:
            memo[key] = nat.assemble_backward_supported(key[0], key[1], key[2])
        return memo[key]

    def _packed_train_head_ok(self, f, ch, lh):
        """Training step, bf16 autocast on the GPU, 3x3 'same' heads on a map the slab / weight-gradient kernels cover."""
        return (self._fused_train(f, ch) and lh.bias is not None and self._packed_head_ok(ch, lh, f) and f.shape[1] % 128 == 0
                and f.shape[3] <= 190 and not sel.on("NO_OWN_HEADS")
                and ch in self.conf_heads and self._packed_head_shadow(list(self.conf_heads).index(ch)) is not None)

    def _heads_grouped(self, feats):
        outs = nat.conv2d_same_group(list(feats), [self._packed_head_weight(l) for l in range(len(feats))], None, relu=False)
        return outs, [None] * len(outs)

    def _heads_halo_grouped(self, feats):
        """All packed heads through the slab kernel in one launch of persistent workgroups (csrc/ssdhip_convh.hip): filters padded to a
        multiple of 128 output channels; the deepest head (fc7's: 144 K-steps) is dispatched first."""
        outs = nat.conv3x3_halo_group(list(feats), [self._packed_head_weight(l, 128) for l in range(len(feats))], None, relu=False)
        return outs, [None] * len(outs)

    def _heads_halo_mixed(self, feats):
        """Round 6, fourth session (SSD512: its conv4_3 map is 64 wide, two columns more than the grouped slab launch's LDS layout takes,
        and ALL seven heads fell back to the implicit-GEMM group -- 223 us of a 3.0 ms step): the maps wider than 62 each through the
        single-problem slab entry (which tiles them as it sees fit: 16 x 16-pixel tiles, one round of 256 workgroups at batch 16), the
        others as the grouped slab launch."""
        wide = [l for l, f in enumerate(feats) if f.shape[3] > 62]
        rest = [l for l in range(len(feats)) if l not in wide]
        outs = [None] * len(feats)
        for l in wide:
            outs[l] = nat.conv3x3_halo(feats[l], self._packed_head_weight(l, 128), None, relu=False, pool=False)
        if rest:
            got = nat.conv3x3_halo_group([feats[l] for l in rest], [self._packed_head_weight(l, 128) for l in rest], None, relu=False)
            for l, y in zip(rest, got):
                outs[l] = y
        return outs, [None] * len(outs)

    def _halo_heads_mixed_ok(self, feats):
        rest = [f for f in feats if f.shape[3] <= 62]
        return (not sel.on("NO_HALO") and not sel.on("NO_HALO_MIXED")
                and len(rest) <= 8 and len(rest) < len(feats)
                and all(f.shape[1] % 128 == 0 for f in feats))

    def _halo_heads_ok(self, feats):
        return (not sel.on("NO_HALO") and len(feats) <= 8
                and all(f.shape[1] % 128 == 0 and f.shape[3] <= 62 for f in feats))

    def _heads_per_layer(self, feats):
        """Per layer the two heads run either as two MIOpen convolutions or PACKED into one libssdhip implicit-GEMM launch
        (conf and loc filters concatenated along Cout, zero-padded to 64 channels): timed once per shape, faster kept."""
        confs, locs = [], []
        for l, (f, ch, lh) in enumerate(zip(feats, self.conf_heads, self.loc_heads)):
            cands = {"miopen": lambda f=f, ch=ch, lh=lh: (self._conv_nobias(ch, f), self._conv_nobias(lh, f))}
            if self._packed_head_ok(ch, lh, f):
                cands["igemm"] = lambda f=f, l=l: (nat.conv2d_same(f, self._packed_head_weight(l), None, dilation=1, relu=False), None)
            name = self._pick(("head", l, tuple(f.shape), ch.out_channels, lh.out_channels), cands) if len(cands) > 1 else "miopen"
            c, lo = cands[name]()
            confs.append(c)
            locs.append(lo)
        return confs, locs

    @staticmethod
    def _packed_head_ok(ch, lh, f):
        same = lambda c: (c.kernel_size == (3, 3) and c.stride == (1, 1) and c.padding == (1, 1) and c.dilation == (1, 1) and c.groups == 1)
        return same(ch) and same(lh) and ch.in_channels % 64 == 0 and ch.in_channels == lh.in_channels

    def _packed_head_weight(self, l, multiple=64):
        """[conf filters | loc filters | zero rows up to a multiple of `multiple`] of predictor layer l as one (Cout, Cin, 3, 3) bf16
        weight in channels_last memory; rebuilt when either head's weight tensor changes (in-place updates bump `_version`)."""
        ch, lh = self.conf_heads[l], self.loc_heads[l]
        key = (ch.weight._version, lh.weight._version, ch.weight.data_ptr(), lh.weight.data_ptr())
        hit = self._packed_heads.get((l, multiple))
        n = ch.out_channels + lh.out_channels
        if hit is not None and hit[0] != key and hit[1].device == ch.weight.device and hit[1].dtype == ch.weight.dtype:
            # refreshed IN PLACE: a captured HIP graph (GraphedInference) keeps reading this storage
            with torch.no_grad():
                hit[1][:ch.out_channels].copy_(ch.weight)
                hit[1][ch.out_channels:n].copy_(lh.weight)
            hit = (key, hit[1])
            self._packed_heads[(l, multiple)] = hit
        elif hit is None or hit[0] != key:
            pad = (-n) % multiple
            with torch.no_grad():
                w = torch.cat([ch.weight, lh.weight] + ([ch.weight.new_zeros((pad,) + tuple(ch.weight.shape[1:]))] if pad else []), dim=0)
                w = w.contiguous(memory_format=torch.channels_last)
            hit = (key, w)
            self._packed_heads[(l, multiple)] = hit
        return hit[1]

    def _head_weights_key(self):
        return tuple((c.weight._version, c.weight.data_ptr()) for heads in (self.conf_heads, self.loc_heads) for c in heads)

    def _refresh_packed_heads(self):
        """Rebuild every cached packed head filter IN ITS OWN STORAGE (a captured HIP graph keeps reading that storage)."""
        for (l, multiple) in list(self._packed_heads):
            self._packed_head_weight(l, multiple)
