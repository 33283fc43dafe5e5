"""The training loop of the prompt learners (`coop.run_coop`, `vpt.run_vpt`, `maple.run_maple`, `cocoop.run_cocoop`, `prograd.run_prograd`,
`promptsrc.run_promptsrc`), stated once: SGD with momentum on a few fp32 tensors,
a cosine schedule over every step, torch's GradScaler in front of the fp16 gradient stream of the towers, one seeded permutation of the samples per epoch."""
import numpy as np
import torch


def accuracy(pred, labels):
    return 100.0 * float((pred == labels.to(pred.device).long()).sum().item()) / labels.shape[0]


def train_prompts(name, parameters, loss_at, n_samples, device, *, epochs, batch, lr, momentum, loss_scale, seed, evaluate=None, backward=None,
                  on_epoch_end=None):
    """`epochs` passes over `n_samples` samples in batches of `batch`: loss_at(idx) -> the loss of the samples idx (an int64 index tensor on `device`);
    evaluate() -> the test accuracy in per cent, printed (under `name`) before training and after every epoch.  Per step: zero_grad, scaled backward,
    step, scaler update, scheduler step.  backward(loss, scaler): a step of its own in place of `scaler.scale(loss).backward()` — it leaves the SCALED
    gradients in `.grad` and calls `scaler.scale` at least once (ProGrad's two walks and projection); None: that line.  on_epoch_end(epoch): called after
    the last step of epoch 0, 1, .., before that epoch's evaluation (PromptSRC's running aggregate of the parameters); None: nothing.  Returns (results, per-epoch mean losses); results = {"epochs": [{"loss", "test_acc"}], "start_test_acc"}, the
    accuracies only with `evaluate`."""
    steps = (n_samples + batch - 1) // batch
    optimizer = torch.optim.SGD(parameters, lr=lr, momentum=momentum)
    scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, max(1, epochs * steps))
    scaler = torch.amp.GradScaler("cuda", init_scale=float(loss_scale))
    res = {"epochs": []}
    if evaluate is not None:
        res["start_test_acc"] = evaluate()
        print("\n**** {}'s test accuracy before training: {:.2f}. ****\n".format(name, res["start_test_acc"]))
    g = torch.Generator().manual_seed(seed)
    epoch_losses = []
    for epoch in range(epochs):
        print("Train Epoch: {:} / {:}".format(epoch, epochs))
        order = torch.randperm(n_samples, generator=g).to(device)
        losses = []
        for s in range(steps):
            loss = loss_at(order[s * batch:(s + 1) * batch])
            optimizer.zero_grad()
            if backward is None:
                scaler.scale(loss).backward()
            else:
                backward(loss, scaler)
            scaler.step(optimizer)
            scaler.update()
            scheduler.step()
            losses.append(float(loss.detach()))
        epoch_losses.append(float(np.mean(losses)))
        print("LR: {:.6f}, Loss: {:.4f}".format(scheduler.get_last_lr()[0], epoch_losses[-1]))
        if on_epoch_end is not None:
            on_epoch_end(epoch)
        rec = {"loss": epoch_losses[-1]}
        if evaluate is not None:
            rec["test_acc"] = evaluate()
            print("**** {}'s test accuracy: {:.2f}. ****\n".format(name, rec["test_acc"]))
        res["epochs"].append(rec)
    return res, epoch_losses
