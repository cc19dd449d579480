/* pool.c -- see pool.h */
#include "pool.h"
#include "cli.h"

struct pool {
    pthread_mutex_t mu;
    pthread_cond_t go, done;
    pthread_t *th;
    int nworkers;        /* threads besides the caller */
    uint64_t epoch;      /* bumped for every pfor call */
    int running;         /* workers still inside the current call */
    int quit;
    pfor_fn fn;
    void *ctx;
    uint32_t n, next;
};
typedef struct {
    pool_t *pool;
    int tid;
} pool_worker_t;

static void pool_drain(pool_t *p, int tid) {
    for (;;) {
        const uint32_t i = __atomic_fetch_add(&p->next, 1u, __ATOMIC_RELAXED);
        if (i >= p->n) break;
        p->fn(p->ctx, i, tid);
    }
}
static void *pool_worker(void *a_) {
    pool_worker_t *w = (pool_worker_t *)a_;
    pool_t *p = w->pool;
    uint64_t seen = 0;
    pthread_mutex_lock(&p->mu);
    for (;;) {
        while (!p->quit && p->epoch == seen) pthread_cond_wait(&p->go, &p->mu);
        if (p->quit) break;
        seen = p->epoch;
        pthread_mutex_unlock(&p->mu);
        pool_drain(p, w->tid);
        pthread_mutex_lock(&p->mu);
        if (--p->running == 0) pthread_cond_signal(&p->done);
    }
    pthread_mutex_unlock(&p->mu);
    free(w);
    return NULL;
}
pool_t *pool_create(int nthreads) {
    pool_t *p = (pool_t *)calloc(1, sizeof *p);
    if (!p) die_mem();
    pthread_mutex_init(&p->mu, NULL);
    pthread_cond_init(&p->go, NULL);
    pthread_cond_init(&p->done, NULL);
    p->nworkers = nthreads > 1 ? nthreads - 1 : 0;
    p->th = (pthread_t *)calloc((size_t)p->nworkers + 1, sizeof(pthread_t));
    if (!p->th) die_mem();
    for (int t = 0; t < p->nworkers; t++) {
        pool_worker_t *w = (pool_worker_t *)malloc(sizeof *w);
        if (!w) die_mem();
        w->pool = p;
        w->tid = t + 1;
        if (pthread_create(&p->th[t], NULL, pool_worker, w) != 0) {
            ERROR("pool", "%s", "cannot create thread");
            die_now();
        }
    }
    return p;
}
void pool_destroy(pool_t *p) {
    pthread_mutex_lock(&p->mu);
    p->quit = 1;
    pthread_cond_broadcast(&p->go);
    pthread_mutex_unlock(&p->mu);
    for (int t = 0; t < p->nworkers; t++) pthread_join(p->th[t], NULL);
    free(p->th);
    free(p);
}
void pfor(pool_t *p, uint32_t n, pfor_fn fn, void *ctx) {
    if (n == 0) return;
    pthread_mutex_lock(&p->mu);
    p->fn = fn; p->ctx = ctx; p->n = n; p->next = 0;
    p->running = p->nworkers;
    p->epoch++;
    pthread_cond_broadcast(&p->go);
    pthread_mutex_unlock(&p->mu);
    pool_drain(p, 0);
    pthread_mutex_lock(&p->mu);
    while (p->running > 0) pthread_cond_wait(&p->done, &p->mu);
    pthread_mutex_unlock(&p->mu);
}

void q_init(queue_t *q) {
    pthread_mutex_init(&q->mu, NULL);
    pthread_cond_init(&q->cv, NULL);
    q->head = q->tail = NULL;
}
void q_push(queue_t *q, qnode_t *x) {
    pthread_mutex_lock(&q->mu);
    x->next = NULL;
    if (q->tail) q->tail->next = x;
    else q->head = x;
    q->tail = x;
    pthread_cond_signal(&q->cv);
    pthread_mutex_unlock(&q->mu);
}
static qnode_t *q_take(queue_t *q) {   /* under the lock */
    qnode_t *x = q->head;
    if (x) {
        q->head = x->next;
        if (!q->head) q->tail = NULL;
    }
    return x;
}
qnode_t *q_pop(queue_t *q) {
    pthread_mutex_lock(&q->mu);
    while (!q->head) pthread_cond_wait(&q->cv, &q->mu);
    qnode_t *x = q_take(q);
    pthread_mutex_unlock(&q->mu);
    return x;
}
qnode_t *q_try_pop(queue_t *q) {
    pthread_mutex_lock(&q->mu);
    qnode_t *x = q_take(q);
    pthread_mutex_unlock(&q->mu);
    return x;
}
