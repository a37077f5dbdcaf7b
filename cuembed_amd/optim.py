"""Sparse optimizers on the compressed gradient (an extension: the reference ends at the gradient).

Two ways in, both ending in the same HIP kernels (cuembed_amd.ops.sparse_row_update; cuembed_amd.ops.sparse_row_adam for
the Adam family):

    SparseUpdater(table, rule, lr)              owns the optimizer state and applies (ids, rows) gradients to the
        .apply(ids, rows, count=... | last_id=... | counts=..., piece_rows=...)      table in place;
        .backward_and_apply(out_grad, idx, offsets, weights)   the whole backward of a sum-pooled lookup + the
                                                update, with the row count left on the device: no host read-back, so
                                                forward + backward_and_apply can be captured into a HIP graph;
      SparseGradResult.apply_to(updater)        feeds it the pieces of SparseGradExchange (cuembed_amd.distributed).

    SparseSGD / SparseAdagrad / RowwiseAdagrad  torch.optim.Optimizer subclasses for parameters whose .grad is the
                                                COALESCED sparse COO tensor of
                                                cuemb_embedding(..., sparse_grad=True | "reference" | "blocked").
                                                An uncoalesced or dense gradient is an error, never coalesced silently.
                                                (autograd drops the tensor's is_coalesced flag on the way into .grad;
                                                step() then checks that the row ids ascend strictly, which reads one
                                                byte back -- those gradient kinds read the row count back anyway.)

Rules (fp32 arithmetic whatever the table's dtype, one rounding to it at the store):
    "sgd"              w <- w - lr * g
    "adagrad"          s <- s + g^2;  w <- w - lr * g / (sqrt(s) + eps)      (torch.optim.Adagrad, lr_decay = 0,
                                                                              weight_decay = 0); fp32 state [rows, W]
    "rowwise_adagrad"  s_r <- s_r + mean_j(g_j^2);  w_j <- w_j - lr * g_j / (sqrt(s_r) + eps);  fp32 state [rows]
No momentum, weight decay or lr_decay for these three.

The Adam family has entries of its own (two state tensors, more hyper-parameters):

    SparseAdamUpdater(table, lr, betas, eps, weight_decay, rowwise=False, bias_correction=True)
        .apply(...) / .backward_and_apply(...)  as SparseUpdater's; owns exp_avg, exp_avg_sq (fp32) and a bias-factor clock
                                                on the device that every apply advances there: still capturable;
    SparseAdam / RowwiseAdam                    torch.optim.Optimizer subclasses for coalesced sparse gradients, with
                                                torch.optim.SparseAdam's state keys ("step", "exp_avg", "exp_avg_sq").

    "adam"          w <- w - (lr * weight_decay) * w  (if weight_decay != 0: decoupled, named rows only)
                    m <- beta1 * m + (1 - beta1) * g;  v <- beta2 * v + (1 - beta2) * g^2       fp32 state 2 x [rows, W]
                    w <- w - (lr * c) * m / (sqrt(v) + eps),  c = sqrt(1 - beta2^t) / (1 - beta1^t)
                    (torch.optim.SparseAdam's formula; lazy: the moments of rows that are not named do not decay)
    "rowwise_adam"  m as above;  v_r <- beta2 * v_r + (1 - beta2) * mean_j(g_j^2);  w_j <- w_j - (lr * c) / (sqrt(v_r) + eps) * m_j
                    fp32 state [rows, W] + [rows]

A GROUP of tables held as separate tensors (cuembed_amd.grouped.TableGroup) is stepped in ONE launch, whatever the
number of tables, by

    GroupSparseUpdater(group, rule, lr) / GroupSparseAdamUpdater(group, lr, ...)
        .apply(grad)                            a GroupedGrad (cuembed_amd.grouped_backward.embedding_backward_grouped);
        .backward_and_apply(grad_y, idx, offsets, weights, mode)     the grouped backward in its compressed form + the
                                                step: no read-back, so forward + backward_and_apply can be captured.
                                                They own one state tensor (Adam: two) per table.  With
                                                stochastic_rounding=True, seeds=[one per table] (16-bit tables) the step
                                                rounds table t with the bits of (seeds[t], rounding_step, row in the
                                                table, column): those of one SparseUpdater(seed=seeds[t]) per table, and
                                                not those of an updater on a one-storage group's flat tensor, which names
                                                its bits by the global row.  There are no default seeds.

Stochastic rounding (stochastic_rounding=True, seed=...; float16 / bfloat16 tables): the rounding to the table's dtype
goes up or down with the probability of the fp32 value's position between its neighbours, so that updates below half a
unit in the last place are kept on average instead of being rounded away at every step.  The bits are a pure function
of (seed, step, table row, column); the step count lives on the device (SparseUpdater.rounding_step, advanced in place
after every apply, so a captured graph draws fresh bits at every replay) or in the optimizer's state
(state[p]["rounding_step"], carried by state_dict()).
"""
import torch

from . import grouped as _grouped
from . import grouped_backward as _grouped_backward
from . import ops as _ops
from .mixed_group_backward import MixedGroupedGrad

_ACCEPTED = ("the coalesced sparse COO gradient of cuemb_embedding(..., sparse_grad=True | 'reference' | 'blocked'); "
             "for a step without a host read-back (HIP graph capture) use SparseUpdater.backward_and_apply")


def _new_state(table, rule, initial_accumulator_value):
    if rule == "sgd":
        return None
    shape = tuple(table.shape) if rule == "adagrad" else (table.shape[0],)
    return torch.full(shape, float(initial_accumulator_value), dtype=torch.float32, device=table.device)


class _CompressedGradientStep:
    """The index path shared by SparseUpdater and SparseAdamUpdater: the backward of a sum-pooled lookup into buffers this
    object keeps, with the row count left on the device, handed to self.apply(ids, rows, last_id=...).  Needs
    self.table and self._buffers = {}."""

    def _step_buffers(self, nnz, dtype, index_dtype, weighted):
        """Gradient rows / ids of min(nnz, num_categories) entries and the sort's workspace, kept between calls."""
        key = (nnz, dtype, index_dtype, weighted)
        b = self._buffers.get(key)
        if b is None:
            capacity = min(nnz, self.table.shape[0])
            dev = self.table.device
            work = _ops.transpose_workspace_bytes(nnz, index_dtype, dtype if weighted else None)
            b = self._buffers[key] = dict(
                rows=torch.empty((capacity, self.table.shape[1]), dtype=dtype, device=dev),
                ids=torch.empty((capacity,), dtype=index_dtype, device=dev),
                work=torch.empty((max(work, 1),), dtype=torch.uint8, device=dev))
        return b

    def backward_and_apply(self, out_grad, idx, offsets=None, weights=None):
        """The backward of out = sum-pooled lookup(table, idx, offsets[, weights]) and the update, in one go:
        row ids -> transpose (+ compressed ids) -> embedding_backward with the row count left on the device, into
        buffers of min(lookups, num_categories) rows that this object keeps -> the update, which reads the count
        itself.  idx [nnz] with offsets [batch + 1] (CSR, closing entry included), or idx [batch, hotness] with
        offsets=None.  out_grad [batch, width] of the table's dtype.  No host read-back and, after the first call at a
        size, no new device memory besides the index arrays torch's caching allocator recycles."""
        if out_grad.dtype != self.table.dtype:
            raise TypeError("out_grad must have the table's dtype (%s), got %s" % (self.table.dtype, out_grad.dtype))
        if out_grad.dim() != 2 or out_grad.shape[1] != self.table.shape[1]:
            raise ValueError("out_grad must be [batch, width]")
        if offsets is None and idx.dim() != 2:
            raise ValueError("without offsets, idx must be [batch, hotness]")
        nnz = idx.numel()
        if nnz == 0:
            return
        ncat = self.table.shape[0]
        b = self._step_buffers(nnz, out_grad.dtype, idx.dtype, weights is not None)
        out_grad = out_grad.contiguous()
        if offsets is None:
            t_idx, t_sid, t_w, remap = _ops.transpose_fixed_hotness(idx.contiguous(), idx.shape[0], idx.shape[1], weights,
                                                                   workspace=b["work"], num_categories=ncat,
                                                                   remapped=True)
        else:
            sid = _ops.extract_row_ids_from_csr(offsets, nnz=nnz, dtype=idx.dtype, batch_size=offsets.numel() - 1)
            t_idx, t_sid, t_w, remap = _ops.transpose(sid, idx.contiguous(), weights, workspace=b["work"],
                                                      num_categories=ncat, remapped=True)
        _ops.embedding_backward(out_grad, None, t_idx, t_sid, remap, t_w, grad_embedding=b["rows"],
                                inverse_mapping=b["ids"])
        self.apply(b["ids"], b["rows"], last_id=remap[nnz - 1:])


class SparseUpdater(_CompressedGradientStep):
    """Applies compressed gradients to `table` ([num_categories, width]; fp32, fp16 or bf16) in place and owns the
    optimizer state (`.state`: None, fp32 [num_categories, width] or fp32 [num_categories]).

    lr is a float or a one-element fp32 device tensor that the kernel reads (fill it to follow a schedule inside a
    captured graph); assign `.lr` to change it.

    stochastic_rounding=True (16-bit tables): every apply rounds stochastically with the bits of (seed, rounding_step),
    where `.rounding_step` is an int64 device word that starts at 0 and is advanced on the device after every apply --
    nothing is read back, so backward_and_apply stays capturable."""

    def __init__(self, table, rule, lr, eps=1e-8, initial_accumulator_value=0.0, stochastic_rounding=False, seed=0):
        if not isinstance(table, torch.Tensor) or table.dim() != 2:
            raise TypeError("table must be a [num_categories, width] tensor")
        if rule not in _ops.UPDATE_RULES:
            raise ValueError("rule must be one of %r, got %r" % (sorted(_ops.UPDATE_RULES), rule))
        if table.dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise TypeError("table must be float32, float16 or bfloat16, got %s" % table.dtype)
        if not table.is_contiguous():
            raise ValueError("table must be contiguous")
        self.table = table.detach()     # (a Parameter is updated through its data)
        self.rule = rule
        self.lr = lr
        self.eps = float(eps)
        self.state = _new_state(table, rule, initial_accumulator_value)
        self._buffers = {}
        self.stochastic_rounding = bool(stochastic_rounding)
        self.seed = seed
        self.rounding_step = None
        if self.stochastic_rounding:
            _check_rounding(table, seed)
            self.rounding_step = torch.zeros((1,), dtype=torch.int64, device=table.device)

    def apply(self, ids, rows, count=None, last_id=None, counts=None, piece_rows=None):
        """table[ids[k]] (and its state) <- rule, for the valid entries of a COALESCED gradient (ids, rows): see
        cuembed_amd.ops.sparse_row_update for the count sources.  Nothing is read back."""
        if not self.stochastic_rounding:
            _ops.sparse_row_update(self.table, ids, rows, rule=self.rule, lr=self.lr, state=self.state, eps=self.eps,
                                   count=count, last_id=last_id, counts=counts, piece_rows=piece_rows)
            return
        _ops.sparse_row_update(self.table, ids, rows, rule=self.rule, lr=self.lr, state=self.state, eps=self.eps,
                               count=count, last_id=last_id, counts=counts, piece_rows=piece_rows,
                               stochastic_rounding=True, seed=self.seed, step=self.rounding_step)
        self.rounding_step.add_(1)      # on the device, after the kernel in stream order: one apply = one step


class SparseAdamUpdater(_CompressedGradientStep):
    """SparseUpdater's counterpart for the Adam family (cuembed_amd.ops.sparse_row_adam): applies compressed gradients to
    `table` in place and owns the moments (`.exp_avg` fp32 [num_categories, width]; `.exp_avg_sq` the same, or fp32
    [num_categories] with rowwise=True) and the bias-factor clock (`.powers` float64 [3] = (t, beta1^t, beta2^t),
    `.bias_factor` float32 [1]), all on the table's device.

    Every apply first advances the clock ON THE DEVICE and then updates with the bias factor the kernel reads from it,
    so that a captured forward + backward_and_apply takes the next step at every replay.  bias_correction=False leaves
    the factor at 1 (the clock still counts).  Only named rows are touched: the moments of other rows do not decay.
    weight_decay is decoupled (AdamW style) and acts on the named rows only.  lr and stochastic_rounding / seed /
    `.rounding_step` are SparseUpdater's."""

    def __init__(self, table, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, rowwise=False, bias_correction=True,
                 stochastic_rounding=False, seed=0):
        if not isinstance(table, torch.Tensor) or table.dim() != 2:
            raise TypeError("table must be a [num_categories, width] tensor")
        if table.dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise TypeError("table must be float32, float16 or bfloat16, got %s" % table.dtype)
        if not table.is_contiguous():
            raise ValueError("table must be contiguous")
        self.betas = _ops._check_betas(betas)
        if not float(eps) >= 0.0 or not float(weight_decay) >= 0.0:
            raise ValueError("eps and weight_decay must not be negative")
        self.table = table.detach()     # (a Parameter is updated through its data)
        self.lr = lr
        self.eps = float(eps)
        self.weight_decay = float(weight_decay)
        self.rowwise = bool(rowwise)
        self.bias_correction = bool(bias_correction)
        self.exp_avg, self.exp_avg_sq = _new_moments(table, self.rowwise)
        self.powers = torch.tensor([0.0, 1.0, 1.0], dtype=torch.float64, device=table.device)
        self.bias_factor = torch.ones((1,), dtype=torch.float32, device=table.device)
        self._one = None if self.bias_correction else torch.ones((1,), dtype=torch.float32, device=table.device)
        self._buffers = {}
        self.stochastic_rounding = bool(stochastic_rounding)
        self.seed = seed
        self.rounding_step = None
        if self.stochastic_rounding:
            _check_rounding(table, seed)
            self.rounding_step = torch.zeros((1,), dtype=torch.int64, device=table.device)

    def apply(self, ids, rows, count=None, last_id=None, counts=None, piece_rows=None):
        """One Adam step on the valid entries of a COALESCED gradient (ids, rows): the clock moves on, then
        cuembed_amd.ops.sparse_row_adam (see there for the count sources).  Nothing is read back."""
        _ops.adam_clock_advance(self.powers, self.bias_factor, self.betas)
        kw = {}
        if self.stochastic_rounding:
            kw = dict(stochastic_rounding=True, seed=self.seed, step=self.rounding_step)
        _ops.sparse_row_adam(self.table, ids, rows, exp_avg=self.exp_avg, exp_avg_sq=self.exp_avg_sq, lr=self.lr,
                             bias_factor=self.bias_factor if self.bias_correction else self._one, betas=self.betas,
                             eps=self.eps, weight_decay=self.weight_decay, rowwise=self.rowwise, count=count,
                             last_id=last_id, counts=counts, piece_rows=piece_rows, **kw)
        if self.stochastic_rounding:
            self.rounding_step.add_(1)      # on the device, after the kernel in stream order: one apply = one step


class _GroupedGradientStep:
    """The index path shared by GroupSparseUpdater and GroupSparseAdamUpdater: the grouped backward in its compressed form
    -- global ids, rows, the count left on the device -- handed to self.apply(grad).  Needs self.group."""

    def _init_group(self, group, stochastic_rounding, seeds):
        group = _grouped._as_group(group)
        if group.quantized:
            raise TypeError("a group of fused 8-bit tables has no optimizer step: quantized tables are inference only")
        self.seeds = _grouped_backward._check_seeds(group, stochastic_rounding, seeds)
        self.stochastic_rounding = self.seeds is not None
        self.group = group
        self.rounding_step = None
        if self.stochastic_rounding:
            # the step word and the seeds on the device, now: the first apply may be under capture
            self.rounding_step = torch.zeros((1,), dtype=torch.int64, device=group.device)
            if group.device.type == "cuda":
                _grouped_backward._seeds_tensor(group, self.seeds)

    def _rounding(self):
        """The rounding keywords of one grouped step."""
        if not self.stochastic_rounding:
            return {}
        return dict(stochastic_rounding=True, seeds=self.seeds, step=self.rounding_step)

    def backward_and_apply(self, grad_y, idx, offsets=None, weights=None, mode="sum"):
        """The backward of out = embedding_forward_grouped(group, idx, offsets, weights, mode=mode) and the step, in one
        go: embedding_backward_grouped(dense=False) -- keys, ONE sort, ONE scatter-add, the entry count left on the device
        -- then the grouped step, which reads the count itself.  grad_y [batch, num_tables, width] of the tables' dtype;
        idx [nnz] with offsets [num_tables * batch + 1] (CSR), or idx [num_tables, batch, hotness] with offsets=None.  No
        host read-back: forward + backward_and_apply on separate tensors can be captured into a HIP graph."""
        hot = 0
        if offsets is None:
            if idx.dim() != 3:
                raise ValueError("without offsets, idx must be [num_tables, batch, hotness]")
            hot = idx.shape[2]
        grad = _grouped_backward.embedding_backward_grouped(self.group, grad_y, idx, offsets, weights, num_hots=hot,
                                                            mode=mode)
        self.apply(grad)
        return grad

    def _check_grad(self, grad):
        # (a MixedGroupedGrad is a GroupedGrad whose rows are padded to the widest table: not what the grouped step reads)
        if not isinstance(grad, _grouped_backward.GroupedGrad) or isinstance(grad, MixedGroupedGrad):
            raise TypeError("apply takes the GroupedGrad of embedding_backward_grouped(dense=False), got %s"
                            % type(grad).__name__)
        if grad.row_base != self.group.row_base:
            raise ValueError("the gradient belongs to a group with other row counts")


class GroupSparseUpdater(_GroupedGradientStep):
    """SparseUpdater for a TableGroup (or a list of tables) of SEPARATE tensors: applies a GroupedGrad to all tables in ONE
    launch (cuembed_amd.grouped_backward.sparse_row_update_grouped) and owns the state, `.states`: None ("sgd") or one
    fp32 tensor per table, [rows_t, width] ("adagrad") or [rows_t] ("rowwise_adagrad").  lr: a float or a one-element
    fp32 device tensor; assign `.lr` to change it.  Works on a one-storage group as well (its tables are views of
    group.flat).

    stochastic_rounding=True, seeds=[...] (16-bit tables): one seed per table, ints in [0, 2**64); every apply rounds
    table t with the bits of (seeds[t], rounding_step), where `.rounding_step` is an int64 device word that starts at 0
    and is advanced on the device after every apply -- also one whose gradient has no entries -- so nothing is read back
    and a captured backward_and_apply draws fresh bits at every replay.  stochastic_rounding=True without seeds is an
    error: there are no default seeds."""

    def __init__(self, group, rule, lr, eps=1e-8, initial_accumulator_value=0.0, stochastic_rounding=False, seeds=None):
        if rule not in _ops.UPDATE_RULES:
            raise ValueError("rule must be one of %r, got %r" % (sorted(_ops.UPDATE_RULES), rule))
        self._init_group(group, stochastic_rounding, seeds)
        self.rule = rule
        self.lr = lr
        self.eps = float(eps)
        self.states = None
        if rule != "sgd":
            self.states = tuple(_new_state(t, rule, initial_accumulator_value) for t in self.group.tables)
            if self.group.device.type == "cuda":     # the pointer arrays, now: the first apply may be under capture
                _grouped_backward._state_ptrs(self.group, self.states)
                self.group.row_base_device

    def apply(self, grad):
        """tables[t][r] (and its state) <- rule, for the valid entries of a GroupedGrad.  Nothing is read back."""
        self._check_grad(grad)
        _grouped_backward.sparse_row_update_grouped(self.group, grad.ids, grad.rows, rule=self.rule, lr=self.lr,
                                                    states=self.states, eps=self.eps, last_id=grad.last_id,
                                                    **self._rounding())
        if self.stochastic_rounding:
            self.rounding_step.add_(1)      # on the device, after the kernel in stream order: one apply = one step


class GroupSparseAdamUpdater(_GroupedGradientStep):
    """SparseAdamUpdater for a TableGroup of SEPARATE tensors: one launch for the clock, one for all tables
    (cuembed_amd.grouped_backward.sparse_row_adam_grouped).  Owns `.exp_avg` and `.exp_avg_sq`, one fp32 tensor per table
    each ([rows_t, width]; exp_avg_sq [rows_t] with rowwise=True), and ONE bias-factor clock for the group (`.powers`,
    `.bias_factor`), which every apply advances on the device: a captured step takes the next step at every replay.
    bias_correction=False leaves the factor at 1.  stochastic_rounding / seeds / `.rounding_step` are
    GroupSparseUpdater's."""

    def __init__(self, group, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, rowwise=False, bias_correction=True,
                 stochastic_rounding=False, seeds=None):
        self.betas = _ops._check_betas(betas)
        if not float(eps) >= 0.0 or not float(weight_decay) >= 0.0:
            raise ValueError("eps and weight_decay must not be negative")
        self._init_group(group, stochastic_rounding, seeds)
        self.lr = lr
        self.eps = float(eps)
        self.weight_decay = float(weight_decay)
        self.rowwise = bool(rowwise)
        self.bias_correction = bool(bias_correction)
        moments = [_new_moments(t, self.rowwise) for t in self.group.tables]
        self.exp_avg = tuple(m for m, _ in moments)
        self.exp_avg_sq = tuple(v for _, v in moments)
        dev = self.group.device
        self.powers = torch.tensor([0.0, 1.0, 1.0], dtype=torch.float64, device=dev)
        self.bias_factor = torch.ones((1,), dtype=torch.float32, device=dev)
        self._one = None if self.bias_correction else torch.ones((1,), dtype=torch.float32, device=dev)
        if dev.type == "cuda":     # the pointer arrays, now: the first apply may be under capture
            _grouped_backward._state_ptrs(self.group, self.exp_avg)
            _grouped_backward._state_ptrs(self.group, self.exp_avg_sq)
            self.group.row_base_device

    def apply(self, grad):
        """One Adam step on the valid entries of a GroupedGrad: the clock moves on, then the grouped step."""
        self._check_grad(grad)
        _ops.adam_clock_advance(self.powers, self.bias_factor, self.betas)
        _grouped_backward.sparse_row_adam_grouped(
            self.group, grad.ids, grad.rows, exp_avg=self.exp_avg, exp_avg_sq=self.exp_avg_sq, lr=self.lr,
            bias_factor=self.bias_factor if self.bias_correction else self._one, betas=self.betas, eps=self.eps,
            weight_decay=self.weight_decay, rowwise=self.rowwise, last_id=grad.last_id, **self._rounding())
        if self.stochastic_rounding:
            self.rounding_step.add_(1)      # on the device, after the kernel in stream order: one apply = one step


def _new_moments(table, rowwise):
    exp_avg = torch.zeros(tuple(table.shape), dtype=torch.float32, device=table.device)
    exp_avg_sq = torch.zeros((table.shape[0],) if rowwise else tuple(table.shape), dtype=torch.float32,
                             device=table.device)
    return exp_avg, exp_avg_sq


def _check_rounding(table, seed):
    if table.dtype == torch.float32:
        raise TypeError("stochastic_rounding is for float16 / bfloat16 tables: a float32 table is not rounded")
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 64:
        raise ValueError("seed must be an int in [0, 2**64), got %r" % (seed,))


def _is_coalesced(g):
    """Whether the sparse gradient holds one entry per row.  Autograd drops the is_coalesced flag when it stores a
    sparse gradient in .grad, so a tensor without the flag is looked at: strictly ascending row ids are what
    cuemb_embedding's coalesced kinds deliver (one byte read back; the flag is then set so that it is paid once per
    gradient).  Nothing is ever coalesced here."""
    if g.is_coalesced():
        return True
    ids = g._indices()
    if ids.shape[0] != 1:
        return False
    if ids.shape[1] > 1 and not bool((ids[0, 1:] > ids[0, :-1]).all()):
        return False
    g._coalesced_(True)
    return True


class _SparseOptimizer(torch.optim.Optimizer):
    """Common part of the torch.optim front ends: one SparseUpdater-style state tensor per parameter, kept in
    self.state[p]["sum"] so that state_dict() / load_state_dict() carry it.  With stochastic_rounding=True the number of
    steps taken on a parameter is self.state[p]["rounding_step"] (a Python int: step() reads the gradient's size back
    anyway), so a resumed optimizer continues the same bit stream."""
    _rule = None

    def __init__(self, params, lr, eps=1e-8, initial_accumulator_value=0.0, stochastic_rounding=False, seed=0):
        if not isinstance(lr, torch.Tensor) and lr < 0.0:
            raise ValueError("invalid learning rate: %r" % (lr,))
        if eps < 0.0 or initial_accumulator_value < 0.0:
            raise ValueError("eps and initial_accumulator_value must not be negative")
        super().__init__(params, dict(lr=lr, eps=eps, initial_accumulator_value=initial_accumulator_value,
                                      stochastic_rounding=bool(stochastic_rounding), seed=seed))
        for group in self.param_groups:
            for p in group["params"]:
                if p.dim() != 2:
                    raise ValueError("every parameter must be a [num_categories, width] table")
                if group["stochastic_rounding"]:
                    _check_rounding(p, group["seed"])
                    self.state[p]["rounding_step"] = 0
                if self._rule != "sgd":
                    self.state[p]["sum"] = _new_state(p, self._rule, group["initial_accumulator_value"])

    def load_state_dict(self, state_dict):
        """As torch's, except that the accumulators stay fp32 (torch casts optimizer state to the parameter's dtype,
        which would round the state of a 16-bit table)."""
        super().load_state_dict(state_dict)
        saved = state_dict["state"]
        ids = [i for g in state_dict["param_groups"] for i in g["params"]]
        params = [p for g in self.param_groups for p in g["params"]]
        for i, p in zip(ids, params):
            if i in saved and "sum" in saved[i]:
                self.state[p]["sum"] = saved[i]["sum"].detach().to(device=p.device, dtype=torch.float32).clone()
            if i in saved and "rounding_step" in saved[i]:
                self.state[p]["rounding_step"] = int(saved[i]["rounding_step"])

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if not g.is_sparse:
                    raise ValueError("%s needs a sparse gradient, got a dense one; accepted: %s"
                                     % (type(self).__name__, _ACCEPTED))
                if not _is_coalesced(g):
                    raise ValueError("%s needs a COALESCED sparse gradient (one entry per table row), got an uncoalesced "
                                     "one (sparse_grad='uncoalesced' / 'padded' / 'fastest'); accepted: %s"
                                     % (type(self).__name__, _ACCEPTED))
                if g.sparse_dim() != 1 or g.dense_dim() != 1:
                    raise ValueError("the gradient must have one sparse (row) and one dense (column) dimension")
                state = self.state[p].get("sum") if self._rule != "sgd" else None
                if not group.get("stochastic_rounding", False):
                    _ops.sparse_row_update(p.data, g._indices()[0].contiguous(), g._values().contiguous(),
                                           rule=self._rule, lr=group["lr"], state=state, eps=group["eps"])
                    continue
                step = int(self.state[p].get("rounding_step", 0))
                _ops.sparse_row_update(p.data, g._indices()[0].contiguous(), g._values().contiguous(), rule=self._rule,
                                       lr=group["lr"], state=state, eps=group["eps"], stochastic_rounding=True,
                                       seed=group["seed"], step=step)
                self.state[p]["rounding_step"] = step + 1
        return loss


class SparseSGD(_SparseOptimizer):
    """w <- w - lr * g on the rows of a coalesced sparse gradient (torch.optim.SGD without momentum / weight decay)."""
    _rule = "sgd"

    def __init__(self, params, lr, stochastic_rounding=False, seed=0):
        super().__init__(params, lr, stochastic_rounding=stochastic_rounding, seed=seed)


class SparseAdagrad(_SparseOptimizer):
    """torch.optim.Adagrad (lr_decay = 0, weight_decay = 0) on the rows of a coalesced sparse gradient; the
    accumulator is fp32 whatever the table's dtype."""
    _rule = "adagrad"


class RowwiseAdagrad(_SparseOptimizer):
    """Adagrad with ONE accumulator per table row (the mean of the row's squared gradient): 4 bytes of state per row
    instead of 4 * width."""
    _rule = "rowwise_adagrad"


def _checked_sparse_grad(opt, g):
    """The gradient of a parameter as (ids, rows), or the front ends' errors for dense and uncoalesced ones."""
    if not g.is_sparse:
        raise ValueError("%s needs a sparse gradient, got a dense one; accepted: %s" % (type(opt).__name__, _ACCEPTED))
    if not _is_coalesced(g):
        raise ValueError("%s needs a COALESCED sparse gradient (one entry per table row), got an uncoalesced "
                         "one (sparse_grad='uncoalesced' / 'padded' / 'fastest'); accepted: %s"
                         % (type(opt).__name__, _ACCEPTED))
    if g.sparse_dim() != 1 or g.dense_dim() != 1:
        raise ValueError("the gradient must have one sparse (row) and one dense (column) dimension")
    return g._indices()[0].contiguous(), g._values().contiguous()


class SparseAdam(torch.optim.Optimizer):
    """torch.optim.SparseAdam on the rows of a coalesced sparse gradient, in one HIP launch per parameter: lazy (only
    the named rows and their moments move), bias correction in the step size, eps added to sqrt(v); plus a decoupled
    weight_decay on the named rows (0 = torch's optimizer).  The moments are fp32 whatever the table's dtype.

    State per parameter, under torch.optim.SparseAdam's names: "step" (a Python int: step() reads the gradient's size
    back anyway), "exp_avg", "exp_avg_sq" -- a state dict of torch's optimizer for an fp32 table loads here and the
    reverse.  With stochastic_rounding=True the bits of step t are those of (seed, t - 1)."""
    _rowwise = False

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, bias_correction=True,
                 stochastic_rounding=False, seed=0):
        if not isinstance(lr, torch.Tensor) and lr < 0.0:
            raise ValueError("invalid learning rate: %r" % (lr,))
        betas = _ops._check_betas(betas)
        if eps < 0.0 or weight_decay < 0.0:
            raise ValueError("eps and weight_decay must not be negative")
        # (maximize: torch.optim.SparseAdam's step() looks it up in a group loaded from this optimizer's state dict)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, maximize=False,
                                      bias_correction=bool(bias_correction),
                                      stochastic_rounding=bool(stochastic_rounding), seed=seed))
        for group in self.param_groups:
            for p in group["params"]:
                if p.dim() != 2:
                    raise ValueError("every parameter must be a [num_categories, width] table")
                if group["stochastic_rounding"]:
                    _check_rounding(p, group["seed"])
                st = self.state[p]
                st["step"] = 0
                st["exp_avg"], st["exp_avg_sq"] = _new_moments(p, self._rowwise)

    def load_state_dict(self, state_dict):
        """As torch's, except that the moments stay fp32 (torch casts optimizer state to the parameter's dtype, which
        would round the moments of a 16-bit table) and "step" becomes a Python int again."""
        super().load_state_dict(state_dict)
        saved = state_dict["state"]
        ids = [i for g in state_dict["param_groups"] for i in g["params"]]
        params = [p for g in self.param_groups for p in g["params"]]
        for i, p in zip(ids, params):
            if i not in saved:
                continue
            for name in ("exp_avg", "exp_avg_sq"):
                if name in saved[i]:
                    self.state[p][name] = saved[i][name].detach().to(device=p.device, dtype=torch.float32).clone()
            if "step" in saved[i]:
                self.state[p]["step"] = int(saved[i]["step"])

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                if group.get("maximize", False):
                    raise ValueError("%s does not maximize: negate the loss" % type(self).__name__)
                ids, rows = _checked_sparse_grad(self, p.grad)
                st = self.state[p]
                t = int(st["step"]) + 1
                c = _ops.adam_bias_factor(t, group["betas"]) if group.get("bias_correction", True) else 1.0
                kw = {}
                if group.get("stochastic_rounding", False):
                    kw = dict(stochastic_rounding=True, seed=group["seed"], step=t - 1)
                _ops.sparse_row_adam(p.data, ids, rows, exp_avg=st["exp_avg"], exp_avg_sq=st["exp_avg_sq"],
                                     lr=group["lr"], bias_factor=c, betas=group["betas"], eps=group["eps"],
                                     weight_decay=group.get("weight_decay", 0.0), rowwise=self._rowwise, **kw)
                st["step"] = t
        return loss


class RowwiseAdam(SparseAdam):
    """SparseAdam with ONE second moment per table row (the running mean of the row's mean squared gradient): 4 * width +
    4 bytes of state per row instead of 8 * width.  state[p]["exp_avg_sq"] is fp32 [num_categories]."""
    _rowwise = True
