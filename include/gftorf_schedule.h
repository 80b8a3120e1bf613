/*
 * gftorf_schedule.h -- C ABI of the run's schedule kept on the device: "make iteration `it` current" (train.py:120-129,
 * 146-147) as one launch that a graph can hold (libgftorf_rast.so, gfx950).
 *
 *   gft_schedule_tick   reads the iteration counter, writes the iteration's random background, scatters the iteration's row
 *                       of a table of doubles (learning rates, loss weights) to its destinations, and leaves the counter
 *                       one further: one launch
 *
 * Everything the launch writes is a function of the counter it finds, so a captured tick replays as the next iteration
 * with no host statement in between.  Device pointers unless marked HOST.  Returns 0 on success (gft_last_error()).
 */
#ifndef GFTORF_SCHEDULE_H
#define GFTORF_SCHEDULE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GFT_SCHEDULE_MAX_DESTS 1024     /* destinations of one tick */

/* kinds of a destination */
#define GFT_SCHEDULE_F64 0              /* a double is stored: a learning-rate slot of FusedAdam(capturable=True) */
#define GFT_SCHEDULE_F32 1              /* the double rounded once to float32 is stored: anything else */

/* int64 words of the state block */
#define GFT_SCHEDULE_COUNTER 0          /* the iteration the next tick makes current; the tick leaves it one further */
#define GFT_SCHEDULE_ITERATION 1        /* the iteration the last tick made current, for consumers */
#define GFT_SCHEDULE_TICKET 2           /* zero between launches (its low 32 bits count the launch's finished workgroups) */
#define GFT_SCHEDULE_OVERRUN 3          /* sticky: 1 once a tick found the counter outside the table; never cleared here */
#define GFT_SCHEDULE_OVERRUNS 4         /* the number of such ticks; never cleared here */
#define GFT_SCHEDULE_STATE_WORDS 8

/* One destination of the row: *address = table[row][column], as a double or rounded to float32.  address is aligned to
 * its kind; column lies in [0, C) (a destination with another column is skipped). */
typedef struct gft_schedule_dest {
    void* address;
    int32_t column;
    int32_t kind;
} gft_schedule_dest;

typedef struct gft_schedule {
    int64_t* state;                     /* int64 [GFT_SCHEDULE_STATE_WORDS], 8-byte aligned; belongs to this schedule */
    const double* table;                /* float64 [N, C]; row 0 belongs to iteration first_iter */
    int64_t N;
    int32_t C;
    int32_t D;                          /* destinations, 0..GFT_SCHEDULE_MAX_DESTS */
    int64_t first_iter;
    const gft_schedule_dest* dests;     /* [D], 16-byte aligned; may be NULL when D is 0 */
    float* bg;                          /* float32 [n], or NULL: no background */
    int64_t n;
    int64_t T;                          /* threads of torch's own fill of n elements on this device, see below */
} gft_schedule;

/* it = state[COUNTER], read by every workgroup at its start.  Workgroup 0 writes state[ITERATION] = it and scatters row
 * clamp(it - first_iter, 0, N - 1) to the D destinations; an `it` outside the table also sets state[OVERRUN] and adds one to
 * state[OVERRUNS].  The last workgroup to finish -- known by the ticket word, one relaxed atomic per workgroup -- writes
 * state[COUNTER] = it + 1 and clears the ticket.  Ticks that share a state block must follow one another on one stream.
 *
 * bg: the n floats of `torch.manual_seed(it); torch.rand(n, device=...) * 2 - 1`: Philox4x32-10 with the key `it`; the
 * element e = idx + T (4 j + k), idx in [0, T), k in 0..3, is word k of the block whose counter is {j, idx} (64 bits each);
 * a word v becomes u = 2^-32 + v 2^-32 in float32, u = 1 becomes 0, and the element is 2 u - 1.  T is 256 times the grid of
 * torch's fill: min(multiProcessorCount * (maxThreadsPerMultiProcessor / 256), ceil(n / 256)); T >= 1 is all that is checked.
 * The torch generator is not touched.  No host read, no memset, no atomic but the ticket's. */
int gft_schedule_tick(void* hip_stream, const gft_schedule* schedule /* HOST */);

#ifdef __cplusplus
}
#endif
#endif
